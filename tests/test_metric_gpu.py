"""GPU tests of the metrics: pn2_confusion_update against numpy (argmax with np.argmax semantics, bincount, invalid labels,
exact), inside a captured graph, inside every form of the captured training step (Trainer(track_metrics=True)), and
Trainer.eval_step against an eager inference forward -- including the folded-weight trap of a graph captured before training
steps."""
import numpy as np
import pytest

from test_layers_gpu import T
from test_train_gpu import _batch

pytestmark = pytest.mark.gpu


def _small_hp(pn2):
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16)
    return hp


def _logits_labels(rows, C, seed):
    """integer-valued logits (ties in most rows), NaN / +inf / -inf sprinkled in, a row of -inf, some labels out of range"""
    rs = np.random.RandomState(seed)
    z = rs.randint(-3, 4, (rows, C)).astype(np.float32)
    k = max(1, rows // 40)
    for v in (np.nan, np.inf, -np.inf, np.nan):
        z[rs.randint(0, rows, k), rs.randint(0, C, k)] = v
    z[rows // 2] = -np.inf
    if rows > 3:
        z[1] = np.nan
    lab = rs.randint(0, C, rows).astype(np.int64)
    bad = rs.randint(0, rows, max(1, rows // 30))
    lab[bad] = rs.choice([-1, -7, C, C + 3], len(bad))
    return z, lab


def _expected(z, lab, C):
    pd = np.argmax(z, axis=1)
    ok = (lab >= 0) & (lab < C)
    cm = np.bincount(lab[ok] * C + pd[ok], minlength=C * C).reshape(C, C)
    return pd, cm, int((~ok).sum())


@pytest.mark.parametrize("C", [2, 9, 13, 64])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 4097, 131072, 1048583])
def test_confusion_update_equals_numpy(pn2, cuda, rows, C):
    """pred == np.argmax, matrix == bincount, invalid exact; int32 labels in the first call, int64 (with out-of-range values
    beyond int32) in the second, which accumulates"""
    import torch
    M = pn2.util.metric
    z, lab = _logits_labels(rows, C, rows * 7 + C)
    pd, cm, inv = _expected(z, lab, C)
    cmat = M.ConfusionMatrix(C, device=cuda)
    zt = T(z, cuda)
    pred = cmat.increment_from_logits(zt, T(lab.astype(np.int32), cuda), return_pred=True)
    assert pred.dtype == torch.int32 and tuple(pred.shape) == (rows,)
    np.testing.assert_array_equal(pred.cpu().numpy(), pd)
    np.testing.assert_array_equal(cmat.confusion_matrix, cm)
    assert cmat.num_invalid == inv
    lab64 = lab.copy()
    lab64[lab64 >= C] = (1 << 40) + C   # would wrap to an in-range value if read as int32
    pred2 = cmat.increment_from_logits(zt.view(1, rows, C), T(lab64.reshape(1, rows), cuda), return_pred=True)
    assert tuple(pred2.shape) == (1, rows)
    np.testing.assert_array_equal(pred2.cpu().numpy().reshape(-1), pd)
    np.testing.assert_array_equal(cmat.confusion_matrix, 2 * cm)
    assert cmat.num_invalid == 2 * inv
    assert int(cmat.counts[-1]) == 0  # the dump slot of increment_from_list stays empty
    cmat.reset()
    assert not cmat.confusion_matrix.any() and cmat.num_invalid == 0


def test_confusion_update_limits_and_host_matrix(pn2, cuda):
    M = pn2.util.metric
    z, lab = _logits_labels(100, 65, 1)
    with pytest.raises(pn2._lib.Pn2Error):
        M.ConfusionMatrix(65, device=cuda).increment_from_logits(T(z, cuda), T(lab, cuda))
    # a host matrix counts a device batch on the device and adds it to its array
    z, lab = _logits_labels(5000, 9, 2)
    pd, cm, inv = _expected(z, lab, 9)
    h = M.ConfusionMatrix(9)
    h.increment_from_logits(T(z, cuda), T(lab, cuda))
    np.testing.assert_array_equal(h.confusion_matrix, cm)
    assert h.num_invalid == inv
    # increment_from_list on device tensors stays on the device and drops out-of-range pairs, as on the host
    d = M.ConfusionMatrix(9, device=cuda)
    d.increment_from_list(T(lab, cuda), T(pd, cuda))
    h2 = M.ConfusionMatrix(9)
    h2.increment_from_list(lab, pd)
    np.testing.assert_array_equal(d.confusion_matrix, h2.confusion_matrix)
    np.testing.assert_array_equal(h2.confusion_matrix, cm)
    assert d.num_invalid == 0 and int(d.counts[-1]) == 0
    d.all_reduce_()  # no process group: nothing happens
    np.testing.assert_array_equal(d.confusion_matrix, cm)


def test_confusion_update_in_a_captured_graph(pn2, cuda):
    """captured once, replayed three times: three times the counts, loss sums {3 * loss, 3}"""
    import torch
    M = pn2.util.metric
    C = 9
    z, lab = _logits_labels(131072, C, 3)
    pd, cm, inv = _expected(z, lab, C)
    zt, lt = T(z, cuda), T(lab, cuda)
    loss = torch.tensor(0.625, dtype=torch.float32, device=cuda)
    acc = torch.zeros(2, dtype=torch.float64, device=cuda)
    cmat = M.ConfusionMatrix(C, device=cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        M.confusion_update(zt, lt, confusion=cmat.matrix_tensor, invalid=cmat.invalid_tensor, loss=loss, loss_acc=acc)
    assert not cmat.confusion_matrix.any()  # capturing executes nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cmat.confusion_matrix, 3 * cm)
    assert cmat.num_invalid == 3 * inv
    assert acc.cpu().tolist() == [3 * 0.625, 3.0]


def _count_launches(pn2):
    """wrap the library's pn2_confusion_update: -> (calls list, restore)"""
    lib = pn2._lib.lib
    orig = getattr(lib, "pn2_confusion_update")
    calls = []

    def counted(*a):
        calls.append(a[0])
        return orig(*a)
    setattr(lib, "pn2_confusion_update", counted)
    return calls, lambda: setattr(lib, "pn2_confusion_update", orig)


@pytest.mark.parametrize("key", ["eager", "graph", "split", "split3"])
def test_training_metrics_in_every_step_form(pn2, cuda, key):
    """the configurations of test_captured_training_step_equals_eager with track_metrics=True: after every step the running
    matrix equals the numpy accumulation over last_logits and the labels (exactly), the total is steps * B * N, and
    mean_loss the mean of the returned losses"""
    hp = _small_hp(pn2)
    batches = [_batch(cuda, s) for s in range(3)]
    tr = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=3), capture=(key != "eager"),
                           warmup_eager=2, split_capture=key.startswith("split"), overlap_collective=(key == "split3"),
                           track_metrics=True)
    want = np.zeros((9, 9), np.int64)
    losses = []
    for i in range(5):
        pc, labels, smpw = batches[i % 3]
        losses.append(tr.train_step(pc, labels, smpw))
        _, cm, inv = _expected(tr.last_logits.reshape(-1, 9).cpu().numpy(), labels.cpu().numpy().reshape(-1), 9)
        want += cm
        assert inv == 0
        np.testing.assert_array_equal(tr.train_confusion.confusion_matrix, want)
        assert want.sum() == (i + 1) * 8 * 2048
        m = tr.train_metrics()
        np.testing.assert_allclose(m["mean_loss"], np.mean(losses), rtol=1e-6)
        assert m["steps"] == i + 1 and m["num_invalid"] == 0
        np.testing.assert_array_equal(m["confusion_matrix"], want)
    assert (tr._graph is not None) == (key != "eager") and (tr._graph_late is not None) == (key == "split3")
    h = pn2.util.metric.ConfusionMatrix(9)
    h.confusion_matrix = want
    assert m["accuracy"] == h.get_accuracy() and m["per_class_iou"] == h.get_per_class_ious()
    assert m["mean_iou"] == pytest.approx(h.get_mean_iou(), rel=1e-12)
    tr.reset_metrics()
    m = tr.train_metrics()
    assert m["steps"] == 0 and not m["confusion_matrix"].any()


def test_metrics_off_adds_no_launch_and_on_adds_one_per_recorded_step(pn2, cuda):
    hp = _small_hp(pn2)
    batches = [_batch(cuda, s) for s in range(3)]
    for track, want in ((False, 0), (True, 3)):
        calls, restore = _count_launches(pn2)
        try:
            tr = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=3), warmup_eager=2,
                                   track_metrics=track)
            for i in range(5):  # 2 eager steps, the capture (records the launch once), 2 replays
                tr.train_step(*batches[i % 3])
        finally:
            restore()
        assert len(calls) == want, (track, calls)
        assert (tr.train_confusion is None) == (not track) and (tr.last_logits is None) == (not track)
    with pytest.raises(RuntimeError):
        pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=3)).train_metrics()


def test_reset_metrics_between_staged_steps(pn2, cuda):
    """run-ahead steps (sync=False) with the whole next batch staged -- copy graph + step graph, nothing eager on the trainer's
    stream -- and reset_metrics() between them without any synchronisation: the counts at the end are those of the steps after
    the last reset"""
    import torch
    hp = _small_hp(pn2)
    batches = [_batch(cuda, s) for s in range(3)]
    tr = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=3), warmup_eager=2, track_metrics=True)
    logits, losses, staged = [], [], []
    resets = {3: None, 6: None}
    for i in range(9):
        nb = batches[(i + 1) % 3]
        staged.append(tr._staged_tag is not None)
        loss = tr.train_step(*batches[i % 3], sync=False, next_pc=nb[0], next_labels=nb[1], next_smpw=nb[2])
        # copies on the caller's stream, ordered after this step and before the next one (train_step orders its stream after
        # the caller's)
        logits.append(tr.last_logits.clone())
        losses.append(loss.clone())
        if i in resets:
            tr.reset_metrics()
    torch.cuda.synchronize()
    assert staged[4] and staged[5] and staged[7] and staged[8], staged
    want = np.zeros((9, 9), np.int64)
    for i in range(7, 9):
        want += _expected(logits[i].reshape(-1, 9).cpu().numpy(), batches[i % 3][1].cpu().numpy().reshape(-1), 9)[1]
    m = tr.train_metrics()
    np.testing.assert_array_equal(m["confusion_matrix"], want)
    assert m["steps"] == 2
    np.testing.assert_allclose(m["mean_loss"], np.mean([float(x) for x in losses[7:]]), rtol=1e-6)


def _eager_eval(pn2, tr, pc, labels, smpw):
    import torch
    pn2.util.tf_util.set_default_store(tr.store)
    with torch.no_grad():
        logits = pn2.model.get_model(pc, False, 9, tr.hp)[0].clone()
        loss = float(pn2.model.get_loss(logits, labels, smpw))
    return logits, loss


def test_eval_step_equals_eager_inference_and_touches_nothing(pn2, cuda):
    import torch
    hp = _small_hp(pn2)
    batches = [_batch(cuda, s) for s in range(3)]
    tr = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=4), warmup_eager=2)
    for i in range(4):
        tr.train_step(*batches[i % 3])
    state = [tr.flat_p.clone(), tr.flat_m.clone(), tr.flat_v.clone()] + [v.clone() for v in tr.store.buffers.values()]
    pc, labels, smpw = batches[1]
    ref_logits, ref_loss = _eager_eval(pn2, tr, pc, labels, smpw)
    _, cm, _ = _expected(ref_logits.reshape(-1, 9).cpu().numpy(), labels.cpu().numpy().reshape(-1), 9)
    losses = []
    for k in range(3):  # eager warm-up, capture + replay, replay
        losses.append(tr.eval_step(pc, labels, smpw))
        assert torch.equal(tr.last_eval_logits, ref_logits), k
        np.testing.assert_array_equal(tr.eval_confusion.confusion_matrix, (k + 1) * cm)
    assert tr._eval_graph is not None
    np.testing.assert_allclose(losses, [ref_loss] * 3, rtol=1e-6)
    m = tr.eval_metrics()
    np.testing.assert_allclose(m["mean_loss"], ref_loss, rtol=1e-6)
    assert m["steps"] == 3
    dl = tr.eval_step(pc, labels, smpw, sync=False)
    assert torch.is_tensor(dl) and dl.is_cuda
    np.testing.assert_allclose(float(dl), ref_loss, rtol=1e-6)
    after = [tr.flat_p, tr.flat_m, tr.flat_v] + list(tr.store.buffers.values())
    assert all(torch.equal(a, b) for a, b in zip(state, after))
    tr.reset_eval_metrics()
    assert tr.eval_metrics()["steps"] == 0 and not tr.eval_confusion.confusion_matrix.any()


def test_eval_graph_is_recaptured_after_training_steps(pn2, cuda):
    """train -> eval (eager, then captured) -> five captured train replays -> eval: the later evaluations equal what a cold
    fold cache computes from the current weights and differ from the first -- a graph captured before the replays reads the
    folded weights of its time and must not be replayed after them"""
    import torch
    hp = _small_hp(pn2)
    batches = [_batch(cuda, s) for s in range(3)]
    store = pn2.util.tf_util.VariableStore(device=cuda, seed=5)
    tr = pn2.train.Trainer(hp, 9, store=store, warmup_eager=2)
    for i in range(4):
        tr.train_step(*batches[i % 3])
    pc, labels, smpw = batches[0]
    tr.eval_step(pc, labels, smpw)
    l0 = tr.eval_step(pc, labels, smpw)
    assert tr._eval_graph is not None
    ev0 = tr.last_eval_logits.clone()
    for i in range(4, 9):  # replays only
        tr.train_step(*batches[i % 3])
    outs = []
    for _ in range(3):  # after the weights moved: eager, then capture + replay, then replay
        outs.append((tr.eval_step(pc, labels, smpw), tr.last_eval_logits.clone()))
    store._folded.clear()
    cold_logits, cold_loss = _eager_eval(pn2, tr, pc, labels, smpw)
    for loss, lg in outs:
        assert torch.equal(lg, cold_logits), float((lg - cold_logits).abs().max())
        np.testing.assert_allclose(loss, cold_loss, rtol=1e-6)
    assert float((outs[-1][1] - ev0).abs().max()) > 1e-3 and outs[-1][0] != l0


def test_full_size_step_with_metrics(pn2, cuda):
    """configs[1] scale (B=16, N=8192, semantic.json): the training GEMMs take their streaming kernels at these row counts;
    one eager and one captured step with metrics on"""
    import torch
    B, N = 16, 8192
    pc, labels, smpw = _batch(cuda, 11, b=B, n=N)
    tr = pn2.train.Trainer(dict(pn2.model.SEMANTIC_HYPERPARAMS), 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=0),
                           warmup_eager=1, track_metrics=True)
    losses = [tr.train_step(pc, labels, smpw) for _ in range(2)]
    assert tr._graph is not None and all(np.isfinite(losses))
    m = tr.train_metrics()
    assert m["confusion_matrix"].sum() == 2 * B * N and m["steps"] == 2
    np.testing.assert_allclose(m["mean_loss"], np.mean(losses), rtol=1e-6)
    _, cm, _ = _expected(tr.last_logits.reshape(-1, 9).cpu().numpy(), labels.cpu().numpy().reshape(-1), 9)
    assert cm.sum() == 131072
    loss = tr.eval_step(pc, labels, smpw)
    assert np.isfinite(loss) and tr.eval_confusion.confusion_matrix.sum() == 131072
    torch.cuda.synchronize()
