"""CPU tests of the metrics: util.metric.ConfusionMatrix against the reference's own self-check (util/metric.py __main__),
numpy bincount, print_metrics, the world-2 all-reduce over gloo, and the argument checks of pn2_confusion_update, which
refuse a call before any HIP call (no GPU needed)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def test_reference_self_check(pn2):
    """the 4x4 matrix of util/metric.py __main__, built with increment(): IoU, mean IoU, accuracy with label 0 ignored"""
    ref = np.array([[0, 1, 2, 3], [0, 4, 5, 6], [0, 7, 8, 9], [0, 10, 11, 12]])
    cm = pn2.util.metric.ConfusionMatrix(num_classes=4)
    for gt in range(4):
        for pd in range(4):
            for _ in range(ref[gt, pd]):
                cm.increment(gt, pd)
    assert cm.confusion_matrix.dtype == np.int64
    np.testing.assert_array_equal(cm.confusion_matrix, ref)
    want = np.array([4.0 / (4 + 7 + 10 + 5 + 6), 8.0 / (5 + 8 + 11 + 7 + 9), 12.0 / (6 + 9 + 12 + 10 + 11)])
    np.testing.assert_allclose(cm.get_per_class_ious(), want)
    np.testing.assert_allclose(want, [4 / 32, 8 / 40, 12 / 48])
    assert cm.get_mean_iou() == np.mean(want)
    assert cm.get_accuracy() == 24.0 / 72.0
    assert cm.num_classes == 4 and cm.valid_labels == {0, 1, 2, 3} and cm.num_invalid == 0


def test_increment_raises_and_from_list_drops_bad_labels(pn2):
    C = 5
    cm = pn2.util.metric.ConfusionMatrix(C)
    for gt, pd in ((-1, 0), (5, 0), (0, 5), (2, -3)):
        with pytest.raises(ValueError):
            cm.increment(gt, pd)
    assert not cm.confusion_matrix.any()
    rs = np.random.RandomState(0)
    gt = rs.randint(-2, C + 2, 5000)
    pd = rs.randint(-1, C + 1, 5000)
    cm.increment_from_list(gt, pd)
    cm.increment_from_list(list(gt[:100]), torch.from_numpy(pd[:100]))  # lists and CPU tensors as well
    ok = (gt >= 0) & (gt < C) & (pd >= 0) & (pd < C)
    want = np.bincount(gt[ok] * C + pd[ok], minlength=C * C).reshape(C, C)
    ok1 = ok[:100]
    want += np.bincount(gt[:100][ok1] * C + pd[:100][ok1], minlength=C * C).reshape(C, C)
    np.testing.assert_array_equal(cm.confusion_matrix, want)
    # one increment per pair gives the same matrix
    cm2 = pn2.util.metric.ConfusionMatrix(C)
    for g, p in zip(gt[ok], pd[ok]):
        cm2.increment(int(g), int(p))
    np.testing.assert_array_equal(cm2.confusion_matrix, np.bincount(gt[ok] * C + pd[ok], minlength=C * C).reshape(C, C))
    with pytest.raises(ValueError):
        cm.increment_from_list([1, 2], [1])
    cm.reset()
    assert not cm.confusion_matrix.any()


def test_print_metrics_format_and_label_check(pn2, capsys):
    M = pn2.util.metric
    cm = M.ConfusionMatrix(3)
    cm.increment_from_list([1, 1, 2, 2, 2], [1, 2, 2, 2, 1])
    with pytest.raises(ValueError):
        cm.print_metrics(labels=["a", "b"])
    capsys.readouterr()  # (the reference prints the heading before it checks the labels)
    cm.print_metrics()
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "Confusion matrix:"
    assert out[1] == "    " + " " * 7 + " " + "      0       1       2 "
    assert out[3] == "          1       0       1       1 "
    assert "IoU per class:" in out and "mIoU (ignoring label 0):" in out and "Overall accuracy" in out
    assert float(out[-1]) == 3.0 / 5.0
    assert M.SEMANTIC3D_LABELS_NAMES[0] == "unlabeled" and len(M.SEMANTIC3D_LABELS_NAMES) == 9
    cm9 = M.ConfusionMatrix(9)
    cm9.increment_from_list([1, 2, 8], [1, 2, 8])
    cm9.print_metrics(labels=M.SEMANTIC3D_LABELS_NAMES)
    text = capsys.readouterr().out
    assert "man-made terrain" in text and "scanning artifact" in text
    lines = M.epoch_log_lines(0.5, cm9.get_per_class_ious(), cm9.get_accuracy(), cm9.get_mean_iou())
    assert lines[:3] == ["mean loss: 0.500000", "Overall accuracy : 1.000000", "Average IoU : %f" % (3.0 / 8.0)]
    assert lines[3] == "IoU of man-made terrain : 1.000000" and lines[-1] == "IoU of cars : 1.000000" and len(lines) == 11


def test_confusion_update_argument_checks_need_no_gpu(pn2):
    L = pn2._lib.lib
    nul = None
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    EINVAL, ENULL, EUNSUP = -1, -2, -4
    assert L.pn2_confusion_update(0, 9, fake, fake, 0, fake, fake, nul, nul, nul, nul) == EINVAL     # rows > 0
    assert L.pn2_confusion_update(-5, 9, fake, fake, 0, fake, fake, nul, nul, nul, nul) == EINVAL
    assert L.pn2_confusion_update(10, 0, fake, fake, 0, fake, fake, nul, nul, nul, nul) == EINVAL    # num_class > 0
    assert L.pn2_confusion_update(10, 9, fake, fake, 0, nul, nul, nul, nul, nul, nul) == EINVAL      # no output requested
    assert L.pn2_confusion_update(10, 9, fake, fake, 0, nul, fake, nul, fake, nul, nul) == EINVAL    # loss without loss_acc
    assert L.pn2_confusion_update(10, 9, fake, fake, 0, nul, fake, nul, nul, fake, nul) == EINVAL    # loss_acc without loss
    assert L.pn2_confusion_update(10, 65, fake, fake, 0, nul, fake, nul, nul, nul, nul) == EUNSUP    # above 64 classes
    assert L.pn2_confusion_update(10, 9, nul, fake, 0, nul, fake, nul, nul, nul, nul) == ENULL       # logits
    assert L.pn2_confusion_update(10, 9, fake, nul, 1, nul, fake, nul, nul, nul, nul) == ENULL       # labels
    assert L.pn2_confusion_update(10, 9, nul, nul, 0, nul, nul, fake, nul, nul, nul) == ENULL       # invalid alone is an output
    assert L.pn2_confusion_update(10, 9, nul, nul, 0, nul, nul, nul, fake, fake, nul) == ENULL       # loss sums alone too
    assert b"PN2_EUNSUP" in L.pn2_strerror(EUNSUP)


def test_device_matrix_needs_cuda_tensors(pn2):
    """increment_from_logits has no CPU path: a CPU tensor is refused, not counted in numpy"""
    cm = pn2.util.metric.ConfusionMatrix(4)
    with pytest.raises(ValueError):
        cm.increment_from_logits(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        cm.increment_from_logits(torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64))  # class count differs


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import pn2_amd as pn2
    pn2.dist.init_from_env(backend="gloo")
    cm = pn2.util.metric.ConfusionMatrix(3)
    cm.increment_from_list([1, 2, 2, 0][:2 + rank], [1, 2, 1, 0][:2 + rank])
    cm._invalid = rank + 1
    before = cm.confusion_matrix.copy()
    cm.all_reduce_()
    q.put((rank, before.tolist(), cm.confusion_matrix.tolist(), cm.num_invalid))
    pn2.dist.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
def test_world2_gloo_all_reduce_sums_the_counts():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r, (np.array(b), np.array(a), inv)) for r, b, a, inv in (q.get(timeout=150) for _ in range(2)))
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    total = res[0][0] + res[1][0]
    assert total.sum() == 5
    for r in range(2):
        np.testing.assert_array_equal(res[r][1], total)
        assert res[r][2] == 3
    # without a process group it is a no-op
    import pn2_amd as pn2
    cm = pn2.util.metric.ConfusionMatrix(2)
    cm.increment(1, 1)
    cm.all_reduce_()
    assert cm.confusion_matrix.tolist() == [[0, 0], [0, 1]]
