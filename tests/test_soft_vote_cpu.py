"""CPU tests of soft voting (csrc/pn2_soft_vote.hip, pn2_interpolate_scores of csrc/pn2_label_interp.hip): the header's
prototypes, the binding, the refusals of the four entry points with placeholder pointers, and the numpy model of the rules
(tests/soft_vote_ref.py) on cases worked out by hand and against the hard-vote model.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import soft_vote_ref as S  # noqa: E402
import tile_ref as M  # noqa: E402

ARGS = {
    "pn2_softmax_scores": ("rows", "num_class", "logits", "q", "invalid", "stream"),
    "pn2_tile_vote_scores": ("b", "npts", "num_class", "sel", "live", "q", "scores", "dropped", "stream"),
    "pn2_score_labels": ("n", "num_class", "scores", "labels", "confidence", "stream"),
    "pn2_interpolate_scores": ("ns", "nd", "num_class", "sparse_points", "sparse_scores", "dense_points", "dense_labels",
                               "dense_colors", "dense_confidence", "knn", "workspace", "workspace_bytes", "stream"),
}


def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    for name, args in ARGS.items():
        assert fns[name].restype is ctypes.c_int and fns[name].argnames == args, name
        assert name in pn2._lib.SIGNATURES and name not in pn2._lib._TRACE_ARGS
    i, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert fns["pn2_softmax_scores"].argtypes == [i, i, p, p, p, p]
    assert fns["pn2_tile_vote_scores"].argtypes == [i, i, i, p, p, p, p, p, p]
    assert fns["pn2_score_labels"].argtypes == [i, i, p, p, p, p]
    assert fns["pn2_interpolate_scores"].argtypes == [i, i, i, p, p, p, p, p, p, i, p, z, p]
    assert "pn2_tile_vote_scores" in pn2._lib._STATEFUL  # it adds into the caller's scores
    assert not {"pn2_softmax_scores", "pn2_score_labels", "pn2_interpolate_scores"} & pn2._lib._STATEFUL
    assert pn2._lib.ABI.constants["PN2_ABI_VERSION"] == 2 and pn2._lib.lib.pn2_abi_version() == 2
    # no new size query: the dense step shares the label form's
    assert sum(f.restype is z for f in fns.values()) == 8
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for name in ARGS:
        assert hasattr(lib, name), name


def _caller(pn2, name, good):
    names = pn2._lib.ABI.functions[name].argnames

    def call(**change):
        a = dict(good, **change)
        return getattr(pn2._lib.lib, name)(*[a[k] for k in names])
    return call


def test_argument_errors_are_refused_without_a_gpu(pn2):
    K = pn2._lib.ABI.constants
    EINVAL, ENULL, ERANGE, EUNSUP = K["PN2_EINVAL"], K["PN2_ENULL"], K["PN2_ERANGE"], K["PN2_EUNSUP"]
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before a launch
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)  # noqa: E731

    soft = _caller(pn2, "pn2_softmax_scores", dict(rows=100, num_class=9, logits=fake, q=fake, invalid=fake, stream=None))
    for bad in (dict(rows=0), dict(rows=-1), dict(num_class=0)):
        assert soft(**bad) == EINVAL, bad
    assert soft(num_class=65) == EUNSUP
    assert soft(logits=None) == ENULL and soft(q=None) == ENULL
    for name, k in (("logits", 2), ("q", 1), ("invalid", 4)):
        assert soft(**{name: odd(k)}) == EINVAL, name
    assert soft(rows=0, logits=None) == EINVAL and soft(num_class=65, q=None) == EUNSUP and soft(q=None, logits=odd(2)) == ENULL

    vote = _caller(pn2, "pn2_tile_vote_scores", dict(b=4, npts=64, num_class=9, sel=fake, live=fake, q=fake, scores=fake,
                                                    dropped=fake, stream=None))
    for bad in (dict(b=0), dict(npts=-1), dict(num_class=0)):
        assert vote(**bad) == EINVAL, bad
    assert vote(b=1 << 16, npts=1 << 16) == ERANGE and vote(num_class=65) == EUNSUP
    for required in ("sel", "live", "q", "scores"):
        assert vote(**{required: None}) == ENULL, required
    for name, k in (("sel", 1), ("live", 2), ("q", 3), ("scores", 4), ("dropped", 4)):
        assert vote(**{name: odd(k)}) == EINVAL, name
    # the order: sizes, ranges, num_class, NULL, alignment
    assert vote(b=0, npts=1 << 30, num_class=65) == EINVAL and vote(b=1 << 16, npts=1 << 16, num_class=65) == ERANGE
    assert vote(num_class=65, sel=None) == EUNSUP and vote(sel=None, scores=odd(4)) == ENULL

    labels = _caller(pn2, "pn2_score_labels", dict(n=100, num_class=9, scores=fake, labels=fake, confidence=fake, stream=None))
    assert labels(n=0) == EINVAL and labels(num_class=0) == EINVAL and labels(num_class=65) == EUNSUP
    assert labels(scores=None) == ENULL and labels(labels=None) == ENULL
    assert labels(scores=odd(4)) == EINVAL and labels(labels=odd(1)) == EINVAL and labels(confidence=odd(2)) == EINVAL
    assert labels(num_class=65, scores=None) == EUNSUP and labels(labels=None, scores=odd(4)) == ENULL

    dense = _caller(pn2, "pn2_interpolate_scores", dict(ns=1000, nd=500, num_class=9, sparse_points=fake, sparse_scores=fake,
                                                       dense_points=fake, dense_labels=fake, dense_colors=fake,
                                                       dense_confidence=fake, knn=3, workspace=ctypes.c_void_p(1 << 20),
                                                       workspace_bytes=0, stream=None))
    for bad in (dict(ns=-1), dict(nd=-1), dict(num_class=0), dict(knn=0)):
        assert dense(**bad) == EINVAL, bad
    assert dense(num_class=65) == EUNSUP and dense(knn=17) == EUNSUP
    for required in ("sparse_points", "sparse_scores", "dense_points", "dense_labels", "dense_colors", "workspace"):
        assert dense(**{required: None}) == ENULL, required
    for name, k in (("sparse_points", 2), ("sparse_scores", 4), ("dense_points", 1), ("dense_labels", 2), ("dense_confidence", 2),
                    ("workspace", 128)):
        assert dense(workspace_bytes=1 << 40, **{name: odd(k)}) == EINVAL, name
    assert dense() == EINVAL                                    # the workspace is too small
    assert dense(workspace_bytes=pn2._lib.lib.pn2_interpolate_label_workspace_bytes(1000) - 1) == EINVAL
    assert dense(knn=0, dense_points=None) == EINVAL and dense(knn=17, dense_points=None) == EUNSUP
    assert dense(nd=0, dense_points=None) == 0                  # nothing to label: nothing is looked at, as in the label form


def test_python_side_checks_come_before_the_device(pn2):
    import pytest
    import torch
    f = pn2.tf_ops.tf_interpolate.interpolate_scores_with_color
    with pytest.raises(ValueError, match="MI355X only"):
        f(torch.zeros(4, 3), torch.zeros(4, 9, dtype=torch.int64), torch.zeros(5, 3), 3)
    assert callable(pn2.predict.label_dense_scores) and callable(pn2.predict.Predictor.predict_scores)
    assert callable(pn2.predict.Predictor.predict_proba) and pn2.predict.SCORE_ONE == S.ONE


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_softmax_by_hand():
    inf, nan = np.inf, np.nan
    x = np.array([[0, 0, 0, 0], [5, 5, -inf, -inf], [1000, 0, -3, 100], [nan, 0, 0, 0], [0, inf, 0, 0], [-inf] * 4,
                  [-inf, 2, -inf, -inf]], dtype=np.float32)
    q, invalid = S.softmax_scores(x)
    assert q.dtype == np.int32 and invalid == 3
    assert q.tolist() == [[1 << 28] * 4, [1 << 29, 1 << 29, 0, 0], [1 << 30, 0, 0, 0], [0] * 4, [0] * 4, [0] * 4, [0, 1 << 30, 0, 0]]
    # log 3 against 0: p = 3/4, 1/4 up to the rounding of float32(log 3) -- far inside one unit of 2^-30 * 2^7
    q, _ = S.softmax_scores(np.array([[np.log(3.0), 0.0]], dtype=np.float32))
    assert abs(int(q[0, 0]) - 3 * (1 << 28)) < 128 and abs(int(q[0].sum()) - S.ONE) <= 1


def test_vote_labels_and_confidence_by_hand():
    """three points, C = 3; sample 0 has 2 live rows, sample 1 has 3.  Row (0,0) -> point 0, (0,1) -> point 1, (0,2) ignored;
    (1,0) -> point 0, (1,1) has a negative entry (dropped whole), (1,2) has sel = -1 (dropped)."""
    scores = np.zeros((3, 3), dtype=np.int64)
    sel = np.array([[0, 1, 2], [0, 1, -1]], dtype=np.int32)
    q = np.array([[[10, 20, 30], [5, 0, 5], [99, 99, 99]], [[1, 2, 3], [7, -1, 7], [4, 4, 4]]], dtype=np.int32)
    assert S.vote_scores(scores, sel, np.array([2, 3], dtype=np.int32), q) == 2
    assert scores.tolist() == [[11, 22, 33], [5, 0, 5], [0, 0, 0]]
    lab, conf = S.score_labels(scores)
    assert lab.tolist() == [2, 0, 0] and lab.dtype == np.int32 and conf.dtype == np.float32
    assert conf.tolist() == [np.float32(0.5), np.float32(0.5), 0.0]


def test_one_hot_scores_are_the_hard_votes():
    """q = 2^30 * onehot(pred): the soft rule adds 2^30 where the hard rule adds 1, drops the same rows, and gives the same labels"""
    rs = np.random.RandomState(11)
    n, b, npts, C = 300, 5, 64, 9
    votes, scores = np.zeros((n, C), dtype=np.int32), np.zeros((n, C), dtype=np.int64)
    for _ in range(3):
        sel = rs.randint(-1, n, (b, npts)).astype(np.int32)
        live = rs.randint(0, npts + 1, b).astype(np.int32)
        pred = rs.randint(0, C, (b, npts)).astype(np.int32)
        q = (np.eye(C, dtype=np.int64)[pred] * S.ONE).astype(np.int32)
        assert M.vote(votes, sel, live, pred) == S.vote_scores(scores, sel, live, q)
    assert votes.sum() > 0 and np.array_equal(scores, votes.astype(np.int64) * S.ONE)
    assert np.array_equal(S.score_labels(scores)[0], M.labels(votes))


def test_dense_model_by_hand():
    """sparse points on the x axis at 0, 1, 2, 3 (point 1 twice: an index tie); dense points at 0.9 and 10"""
    sp = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], dtype=np.float32)
    dp = np.array([[0.9, 0, 0], [10, 0, 0]], dtype=np.float32)
    assert S.neighbours(sp, dp, 3).tolist() == [[1, 2, 0], [4, 3, 1]]
    assert S.neighbours(sp[:2], dp, 3).tolist() == [[1, 0], [1, 0]]
    sc = np.array([[5, 0], [0, 2], [0, 2], [0, 9], [3, 0]], dtype=np.int64)
    lab, col, conf = S.interpolate_scores(sp, sc, dp, 3)  # sums (5, 4) and (3, 11)
    assert lab.tolist() == [0, 1] and col.tolist() == [[255, 255, 255], [0, 0, 255]]
    assert conf.tolist() == [np.float32(5 / 9), np.float32(11 / 14)]
    lab, col, conf = S.interpolate_scores(sp[:0], sc[:0], dp, 3)
    assert lab.tolist() == [-1, -1] and not col.any() and not conf.any()
