"""GPU tests of pn2_label_confusion (csrc/pn2_metric.hip) and of ConfusionMatrix.increment_from_list on it: the matrix and the
count of dropped pairs equal np.bincount exactly at the lane, wave, workgroup and grid-sweep edges, for int32 and int64
labels with out-of-range values on either side, at odd alignment, accumulated over calls, replayed from a graph, and without
torch temporaries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# one lane | the wave edges | the workgroup edges | one full sweep of 256 workgroups x 256 lanes, and the first grid-stride
# step | a ragged many-sweep size
SIZES = [1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 1048583]
POISON = -0x5A5A5A5A5A5A5A5B


def _labels(seed, n, C, label64):
    """gt, pd (numpy, int32 or int64) with out-of-range labels in gt alone, in pd alone and in both, negatives included; int64:
    values whose low word is a class or C itself"""
    rs = np.random.RandomState(seed)
    dt = np.int64 if label64 else np.int32
    gt = rs.randint(0, C, n).astype(dt)
    pd = rs.randint(0, C, n).astype(dt)
    wild = [-1, C, C + 5, -2 ** 31, 2 ** 31 - 1]
    if label64:
        wild += [(1 << 40) + C, (1 << 32) + (C - 1), 1 << 32, -(1 << 35), -(1 << 32) + (C - 1)]
    wild = np.array(wild, dtype=dt)
    kind = rs.randint(0, 8, n)  # 1: gt out of range, 2: pd, 3: both; the rest stays valid
    gt = np.where((kind == 1) | (kind == 3), wild[rs.randint(0, len(wild), n)], gt)
    pd = np.where((kind == 2) | (kind == 3), wild[rs.randint(0, len(wild), n)], pd)
    return gt.astype(dt), pd.astype(dt)


def _want(gt, pd, C):
    g, p = gt.astype(np.int64), pd.astype(np.int64)
    ok = (g >= 0) & (g < C) & (p >= 0) & (p < C)
    return np.bincount(g[ok] * C + p[ok], minlength=C * C).astype(np.int64), int((~ok).sum())


def _guarded(torch, C, dev):
    """the matrix and the dropped count inside a poisoned int64 buffer -> buffer, matrix view, dropped view, mask of the rest"""
    buf = torch.full((C * C + 48,), POISON, dtype=torch.int64, device=dev)
    cm, dr = buf[16:16 + C * C], buf[C * C + 24:C * C + 25]
    cm.zero_()
    dr.zero_()
    rest = torch.ones_like(buf, dtype=torch.bool)
    rest[16:16 + C * C] = False
    rest[C * C + 24] = False
    return buf, cm, dr, rest


def _call(pn2, n, C, gt, pd, cm, dr):
    L = pn2._lib
    L.launch("pn2_label_confusion", gt, n, C, L.ptr(gt), L.ptr(pd), int(gt.dtype.itemsize == 8), L.ptr(cm), L.ptr(dr))


@pytest.mark.parametrize("label64", [0, 1])
@pytest.mark.parametrize("C", [1, 9, 64])
def test_counts_equal_bincount_at_every_edge(pn2, cuda, C, label64):
    import torch
    for k, n in enumerate(SIZES):
        gt_h, pd_h = _labels(100 * C + k, n, C, label64)
        want, want_dropped = _want(gt_h, pd_h, C)
        assert n < 8 or (0 < want_dropped < n and want.sum() + want_dropped == n)  # both kinds of pairs are present
        for odd in (0, 1):  # odd: [1:] slices of a larger tensor -- int32 labels then start 4 bytes off a 16-byte boundary
            if odd:
                gt = torch.from_numpy(np.concatenate([[7], gt_h]).astype(gt_h.dtype)).to(cuda)[1:]
                pd = torch.from_numpy(np.concatenate([[7], pd_h]).astype(pd_h.dtype)).to(cuda)[1:]
                assert gt.data_ptr() % 16 == gt_h.dtype.itemsize
            else:
                gt, pd = torch.from_numpy(gt_h).to(cuda), torch.from_numpy(pd_h).to(cuda)
            buf, cm, dr, rest = _guarded(torch, C, cuda)
            _call(pn2, n, C, gt, pd, cm, dr)
            assert np.array_equal(cm.cpu().numpy(), want), (n, odd)
            assert int(dr.item()) == want_dropped, (n, odd)
            assert bool((buf[rest] == POISON).all()), (n, odd)
            # a second call accumulates; dropped = NULL is accepted and leaves the count alone
            _call(pn2, n, C, gt, pd, cm, None)
            assert np.array_equal(cm.cpu().numpy(), 2 * want), (n, odd)
            assert int(dr.item()) == want_dropped and bool((buf[rest] == POISON).all()), (n, odd)


def test_int64_labels_do_not_wrap(pn2, cuda):
    """every pair below has a class in its low 32 bits and lies outside [0, C) at 64 bits"""
    import torch
    C = 9
    gt = torch.tensor([(1 << 40) + C, (1 << 32) + 3, 3, -(1 << 32) + 2, 4], dtype=torch.int64, device=cuda)
    pd = torch.tensor([3, 3, (1 << 32) + 3, 2, 5], dtype=torch.int64, device=cuda)
    buf, cm, dr, rest = _guarded(torch, C, cuda)
    _call(pn2, 5, C, gt, pd, cm, dr)
    want = np.zeros(C * C, np.int64)
    want[4 * C + 5] = 1
    assert np.array_equal(cm.cpu().numpy(), want) and int(dr.item()) == 4 and bool((buf[rest] == POISON).all())


def test_graph_replays_accumulate(pn2, cuda):
    import torch
    C, n = 9, 65537
    gt_h, pd_h = _labels(5, n, C, 0)
    want, want_dropped = _want(gt_h, pd_h, C)
    gt, pd = torch.from_numpy(gt_h).to(cuda), torch.from_numpy(pd_h).to(cuda)
    buf, cm, dr, rest = _guarded(torch, C, cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(pn2, n, C, gt, pd, cm, dr)
    assert not cm.any()  # the capture launched nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(cm.cpu().numpy(), 3 * want) and int(dr.item()) == 3 * want_dropped
    assert bool((buf[rest] == POISON).all())


def test_more_than_64_classes_are_refused(pn2, cuda):
    import torch
    gt = torch.zeros(16, dtype=torch.int32, device=cuda)
    cm = torch.zeros(65 * 65, dtype=torch.int64, device=cuda)
    with pytest.raises(pn2._lib.Pn2Error, match="pn2_label_confusion"):
        _call(pn2, 16, 65, gt, gt, cm, None)
    assert not cm.any()


def test_increment_from_list_runs_on_the_kernel_without_temporaries(pn2, cuda):
    """contiguous int32 inputs at n = 2^24 go to the kernel as they are: the allocator's peak rises by less than 1 MiB across
    the call.  (Derived, not measured: the torch path this replaces makes at least four int64 tensors of n elements --
    gt.long(), pd.long(), the index, the ones -- 4 * 8 * n = 512 MiB.)"""
    import torch
    C, n = 9, 1 << 24
    gen = torch.Generator(device=cuda)
    gen.manual_seed(3)
    gt = torch.randint(-1, C + 1, (n,), generator=gen, device=cuda, dtype=torch.int32)
    pd = torch.randint(0, C, (n,), generator=gen, device=cuda, dtype=torch.int32)
    want, want_dropped = _want(gt.cpu().numpy(), pd.cpu().numpy(), C)
    cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    cm.increment_from_list(gt, pd)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak allocation across increment_from_list at n = 2^24: +%d bytes" % rise)
    assert rise < (1 << 20)
    assert np.array_equal(cm.confusion_matrix.reshape(-1), want) and want_dropped > 0
    assert cm.num_invalid == 0 and int(cm.counts[-1].item()) == 0  # the C*C + 2 layout: neither extra slot is touched


def test_increment_from_list_casts_other_inputs_once_and_keeps_torch_above_64_classes(pn2, cuda):
    import torch
    rs = np.random.RandomState(4)
    C, n = 9, 5000
    gt_h, pd_h = rs.randint(-2, C + 2, n), rs.randint(-1, C + 1, n)
    want, _ = _want(gt_h, pd_h, C)
    t = lambda a, dt: torch.from_numpy(a.astype(dt)).to(cuda)  # noqa: E731
    for gdt, pdt in ((np.int64, np.int32), (np.int32, np.int64), (np.int16, np.int16), (np.int64, np.int64)):
        cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
        cm.increment_from_list(t(gt_h, gdt).reshape(50, 100), t(pd_h, pdt).reshape(50, 100))
        cm.increment_from_list(t(gt_h, gdt)[::2], t(pd_h, pdt)[::2])  # not contiguous
        w2, _ = _want(gt_h[::2], pd_h[::2], C)
        assert np.array_equal(cm.confusion_matrix.reshape(-1), want + w2), (gdt, pdt)
        assert int(cm.counts[-1].item()) == 0 and cm.num_invalid == 0
    with pytest.raises(ValueError):
        cm.increment_from_list(t(gt_h, np.int32), t(pd_h, np.int32)[:-1])
    C = 70  # above the kernel's limit: the torch lines, as before
    gt_h, pd_h = rs.randint(-2, C + 2, n), rs.randint(-1, C + 1, n)
    cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
    cm.increment_from_list(t(gt_h, np.int32), t(pd_h, np.int64))
    assert np.array_equal(cm.confusion_matrix.reshape(-1), _want(gt_h, pd_h, C)[0])
    assert int(cm.counts[-1].item()) == 0
