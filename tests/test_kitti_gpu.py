"""GPU tests of the KITTI frame flow: pn2_frame_crop and pn2_frame_sample (csrc/pn2_frame.hip) against the numpy model
tests/frame_ref.py, pn2.dataset.KittiFileData / KittiDataset against the fixture frozen from the reference's own code
(tests/golden/kitti_frames.npz), pn2.kitti_predict.PredictInterpolator against the eager colourless model followed by
interpolate_label_with_color, and the file route of examples/predict_kitti.py.

The raw calls write every output into buffers poisoned on both sides; rows the rule leaves unwritten must still hold the poison.
Everything is compared bit for bit: the crop widens float32 exactly, the sampler's float64 subtraction and its one rounding are
the reference's."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0x7FC5A5A5  # a quiet NaN with a payload: an int32 pattern no kernel here writes
GOLDEN = os.path.join(ROOT, "tests", "golden", "kitti_frames.npz")
BOX = F.kitti_box(10, 10)


class Guarded:
    """a tensor of `shape` inside a poisoned allocation; `skew` 4-byte words shift its base off the 256-byte boundary"""

    def __init__(self, torch, dev, shape, dtype, skew=0):
        words = {torch.float32: 1, torch.int32: 1, torch.float64: 2}[dtype]
        n = int(np.prod(shape)) * words
        self.lo, self.hi = 64 + skew, 64 + skew + n
        self.raw = torch.full((self.hi + 64,), POISON, dtype=torch.int32, device=dev)
        self.t = self.raw[self.lo:self.hi].view(dtype).view(*shape)

    def check(self, what, written_words=None):
        """the guards hold; with written_words, so does everything behind the first written_words words of the tensor"""
        assert bool((self.raw[:self.lo] == POISON).all()) and bool((self.raw[self.hi:] == POISON).all()), what + ": guard overwritten"
        if written_words is not None:
            assert bool((self.raw[self.lo + written_words:self.hi] == POISON).all()), what + ": a row past the count was written"


def _ws(pn2, torch, dev, query, n):
    L = pn2._lib
    need = L.u64_array([0])
    L.launch(query, dev, n, need, stream=False)
    ws = torch.empty(int(need[0]) + 256, dtype=torch.uint8, device=dev)
    base = (-ws.data_ptr()) % 256
    return ws[base:base + int(need[0])]


def crop_raw(pn2, dev, frame, lo, hi, skew=0):
    """one raw pn2_frame_crop call, outputs guarded -> points (cnt,3) float64, src (cnt,) int32, as numpy"""
    import torch
    L = pn2._lib
    n, ld = frame.shape
    f = torch.from_numpy(np.ascontiguousarray(frame)).to(dev)
    gp = Guarded(torch, dev, (n, 3), torch.float64, 2 * (skew // 2))
    gs = Guarded(torch, dev, (n,), torch.int32, skew)
    gc = Guarded(torch, dev, (1,), torch.int32, skew)
    ws = _ws(pn2, torch, dev, "pn2_frame_crop_workspace_size", n)
    L.launch("pn2_frame_crop", dev, n, L.ptr(f), ld, *[float(v) for v in lo], *[float(v) for v in hi], L.ptr(gp.t), L.ptr(gs.t),
             L.ptr(gc.t), L.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    cnt = int(gc.t.item())
    what = "n %d ld %d skew %d" % (n, ld, skew)
    assert 0 <= cnt <= n, what
    gp.check(what, cnt * 6)
    gs.check(what, cnt)
    gc.check(what)
    return gp.t[:cnt].cpu().numpy(), gs.t[:cnt].cpu().numpy()


def _same64(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _same32(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _frames(n, ld):
    """the row patterns: name -> (n, ld) float32"""
    rs = np.random.RandomState(n * 7 + ld)
    inside = np.stack([rs.uniform(-5, 5, n), rs.uniform(-5, 5, n), rs.uniform(-2, 5, n)], 1).astype(np.float32)
    outside = inside + np.float32(100.0)
    pad = rs.random_sample((n, ld - 3)).astype(np.float32)
    rows = np.arange(n)[:, None]
    mixed = np.stack([rs.uniform(-8, 8, n), rs.uniform(-8, 8, n), rs.uniform(-4, 7, n)], 1).astype(np.float32)
    pats = {"none": outside, "all": inside, "alternating": np.where(rows % 2 == 0, inside, outside),
            "first": np.where(rows == 0, inside, outside), "last": np.where(rows == n - 1, inside, outside), "mixed": mixed}
    return {k: np.ascontiguousarray(np.concatenate([v, pad], 1)) for k, v in pats.items()}


@pytest.mark.parametrize("ld", [3, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 131075])
def test_crop_row_patterns(pn2, cuda, n, ld):
    for name, frame in _frames(n, ld).items():
        want_p, want_s = F.crop(frame, *BOX)
        got_p, got_s = crop_raw(pn2, cuda, frame, *BOX, skew=(n + ld) % 2)
        assert len(want_s) == {"none": 0, "all": n, "alternating": (n + 1) // 2, "first": 1, "last": 1}.get(name, len(want_s)), name
        assert np.array_equal(got_s, want_s), (name, len(got_s), len(want_s))
        assert _same64(got_p, want_p), name


def _value_rows():
    rows = np.array([[-5, 0, 0], [5, 0, 0], [0, -5, 0], [0, 5, 0], [0, 0, -2], [0, 0, 5]], dtype=np.float32)
    beyond = rows.copy()
    for k in range(6):
        a = k // 2
        beyond[k, a] = np.nextafter(rows[k, a], np.float32(np.inf if rows[k, a] > 0 else -np.inf))
    bad = np.zeros((9, 3), dtype=np.float32)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            bad[3 * k + a, a] = v
    return np.concatenate([rows, beyond, bad, np.array([[-0.0, -0.0, -0.0]], dtype=np.float32)])


@pytest.mark.parametrize("ld", [3, 4])
@pytest.mark.parametrize("reps", [1, 100])
def test_crop_value_edges(pn2, cuda, ld, reps):
    """a value exactly on each of the six bounds is kept, the next float32 beyond it dropped; NaN, +inf and -inf in each coordinate
    drop their row; -0.0 is kept with its sign.  reps = 100: the same rows across three chunks"""
    rows = np.tile(_value_rows(), (reps, 1))
    frame = np.ascontiguousarray(np.concatenate([rows, np.full((len(rows), ld - 3), np.nan, np.float32)], 1))
    got_p, got_s = crop_raw(pn2, cuda, frame, *BOX)
    want_p, want_s = F.crop(frame, *BOX)
    assert list(want_s[:7]) == [0, 1, 2, 3, 4, 5, 21] and len(want_s) == 7 * reps
    assert np.array_equal(got_s, want_s) and _same64(got_p, want_p)
    assert np.signbit(got_p[6]).all()


# ---- sample --------------------------------------------------------------------------------------------------------------
def sample_raw(pn2, dev, pts, npts, bx, by, mask=None, seed=0, counter=None, skew=0):
    """one raw pn2_frame_sample call, outputs guarded -> sel, centered, raw, status as numpy"""
    import torch
    L = pn2._lib
    cnt = len(pts)
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(dev)
    gsel = Guarded(torch, dev, (npts,), torch.int32, skew)
    gcen = Guarded(torch, dev, (npts, 3), torch.float32, skew)
    graw = Guarded(torch, dev, (npts, 3), torch.float64, 2 * (skew // 2))
    gst = Guarded(torch, dev, (1,), torch.int32, skew)
    ws = _ws(pn2, torch, dev, "pn2_frame_sample_workspace_size", cnt)
    ws.fill_(0xA5)  # the call clears what it needs cleared
    L.launch("pn2_frame_sample", dev, cnt, npts, L.ptr(p), L.ptr(m), float(bx), float(by), seed, L.ptr(counter), L.ptr(ws),
             ws.numel(), L.ptr(gsel.t), L.ptr(gcen.t), L.ptr(graw.t), L.ptr(gst.t))
    torch.cuda.synchronize()
    for g in (gsel, gcen, graw, gst):
        g.check("cnt %d npts %d" % (cnt, npts))
    return gsel.t.cpu().numpy(), gcen.t.cpu().numpy(), graw.t.cpu().numpy(), int(gst.t.item())


def _sorted_points(cnt, seed=0):
    rs = np.random.RandomState(100 + cnt + seed)
    p = np.stack([np.sort(rs.uniform(-5, 5, cnt).astype(np.float32)), rs.uniform(-5, 5, cnt).astype(np.float32),
                  rs.uniform(-2, 5, cnt).astype(np.float32)], 1)
    return p.astype(np.float64)


SAMPLE_CASES = [(1, 16), (15, 16), (16, 16), (17, 16), (100, 16), (4097, 1024), (20000, 1024)]


@pytest.mark.parametrize("cnt,npts", SAMPLE_CASES)
def test_sample_replay_equals_the_model(pn2, cuda, cnt, npts):
    pts = _sorted_points(cnt)
    mask = None
    if cnt > npts:
        mask = np.r_[np.ones(npts, np.uint8), np.zeros(cnt - npts, np.uint8)]
        np.random.RandomState(cnt).shuffle(mask)
    else:
        mask = np.ones(cnt, np.uint8)  # ignored: a frame of at most N points is repeated
    sel, cen, raw, st = sample_raw(pn2, cuda, pts, npts, 10, 8, mask=mask, skew=cnt % 2)
    wsel, wcen, wraw, wst = F.sample(pts, npts, 10, 8, mask=mask if cnt > npts else None)
    assert st == wst == 0 and np.array_equal(sel, wsel)
    assert _same64(raw, wraw) and _same32(cen, wcen)
    if cnt > npts:
        for extra in (-1, 1):  # a mask with N - 1 or N + 1 bytes set: status 3, zero-filled outputs
            bad = mask.copy()
            bad[np.nonzero(bad == (1 if extra < 0 else 0))[0][0]] ^= 1
            assert int(bad.sum()) == npts + extra
            sel, cen, raw, st = sample_raw(pn2, cuda, pts, npts, 10, 8, mask=bad)
            assert st == 3 == F.sample(pts, npts, 10, 8, mask=bad)[3]
            assert not sel.any() and not cen.view(np.int32).any() and not raw.view(np.int64).any()


@pytest.mark.parametrize("cnt,npts", SAMPLE_CASES)
def test_sample_device_mode(pn2, cuda, cnt, npts):
    import torch
    pts = _sorted_points(cnt, 1)
    seed, c0 = 7 + cnt, 5
    counter = torch.full((1,), c0, dtype=torch.int64, device=cuda)
    sel, cen, raw, st = sample_raw(pn2, cuda, pts, npts, 10, 10, seed=seed, counter=counter)
    assert int(counter.item()) == c0 + 1  # advanced by exactly one
    wsel, wcen, wraw, wst = F.sample(pts, npts, 10, 10, seed=seed, counter=c0)
    assert st == wst == 0 and np.array_equal(sel, wsel) and _same64(raw, wraw) and _same32(cen, wcen)
    if cnt <= npts:
        assert np.array_equal(sel, np.arange(npts) % cnt)
        return
    assert len(sel) == npts and np.all(np.diff(sel) > 0) and sel[0] >= 0 and sel[-1] < cnt
    nxt = sample_raw(pn2, cuda, pts, npts, 10, 10, seed=seed, counter=counter)  # the next call draws a fresh subset
    assert int(counter.item()) == c0 + 2 and nxt[3] == 0
    assert not np.array_equal(nxt[0], sel) and np.array_equal(nxt[0], F.select(cnt, npts, seed=seed, counter=c0 + 1)[0])
    counter.fill_(c0)  # the same (seed, counter): the same subset
    again = sample_raw(pn2, cuda, pts, npts, 10, 10, seed=seed, counter=counter)
    assert np.array_equal(again[0], sel) and _same32(again[1], cen)
    other = sample_raw(pn2, cuda, pts, npts, 10, 10, seed=seed + 1, counter=counter)
    assert not np.array_equal(other[0], sel)


def dataset_sel_raw(pn2, dev, pts, npts, seed, counter, max_chunks=8):
    """one raw device-mode pn2_dataset_sample call, b = 1, on a one-scene store made of `pts` with half-sizes beyond the scene's
    extent (the column is the whole scene wherever the centre falls) -> out_sel (npts,) as numpy (scene-local: offset 0)"""
    import torch
    L = pn2._lib
    cnt = len(pts)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    p, off, cdf = t(pts, np.float64), t([0, cnt], np.int32), t([1.0], np.float64)
    zsize = t([pts[:, 2].max() - pts[:, 2].min()], np.float64)
    need = L.u64_array([0])
    L.launch("pn2_dataset_workspace_size", dev, 1, max_chunks, need, stream=False)
    ws = torch.zeros(int(need[0]) + 256, dtype=torch.uint8, device=dev)  # the histogram and the candidate count start at zero
    base = (-ws.data_ptr()) % 256
    info = torch.empty((1, 8), dtype=torch.int32, device=dev)
    finfo = torch.empty((1, 3), dtype=torch.float64, device=dev)
    gsel = Guarded(torch, dev, (1, npts), torch.int32)
    data = torch.empty((1, npts, 3), dtype=torch.float32, device=dev)
    lab = torch.empty((1, npts), dtype=torch.int32, device=dev)
    wts = torch.empty((1, npts), dtype=torch.float32, device=dev)
    L.launch("pn2_dataset_sample", dev, 1, npts, 1, max_chunks, 0, 0, L.ptr(p), None, None, L.ptr(off), L.ptr(cdf), L.ptr(zsize),
             None, 0, 100.0, 100.0, seed, L.ptr(counter), None, None, None, 0, None, L.ptr(ws[base:]), int(need[0]), L.ptr(info),
             L.ptr(finfo), L.ptr(gsel.t), L.ptr(data), L.ptr(lab), L.ptr(wts))
    torch.cuda.synchronize()
    gsel.check("cnt %d npts %d" % (cnt, npts))
    info = info.cpu().numpy()[0]
    assert info[7] == 0 and info[2] == cnt, info  # status ok, the column is the whole scene
    return gsel.t[0].cpu().numpy()


@pytest.mark.parametrize("cnt,npts", [(1025, 16), (4097, 1024)])
def test_dataset_and_frame_draw_the_same_subset(pn2, cuda, cnt, npts):
    """one selection behind two entry points: the same (seed, counter) over the same cnt points gives pn2_dataset_sample (b = 1,
    sample 0, a column that is the whole scene) and pn2_frame_sample the same index list.  1025: one row past a chunk; 4097: four
    chunks and one row, about one key per bin, so bin T is populated and the cut decides."""
    import torch
    rs = np.random.RandomState(cnt)
    pts = np.stack([np.arange(cnt) * 0.002 - 4.5, rs.uniform(-5, 5, cnt), rs.uniform(-2, 5, cnt)], 1)  # x strictly ascending
    seed, c0 = 11 + cnt, 3
    counter = torch.full((1,), c0, dtype=torch.int64, device=cuda)
    by_dataset = torch.from_numpy(dataset_sel_raw(pn2, cuda, pts, npts, seed, counter))
    assert int(counter.item()) == c0 + 1
    counter.fill_(c0)
    sel, _, _, st = sample_raw(pn2, cuda, pts, npts, 10, 10, seed=seed, counter=counter)
    assert st == 0
    assert torch.equal(by_dataset, torch.from_numpy(sel))
    assert np.array_equal(sel, F.select(cnt, npts, seed=seed, counter=c0)[0])


def test_centring_uses_the_minimum_of_the_sampled_points(pn2, cuda):
    pts = _sorted_points(100)
    pts[50, 1], pts[50, 2] = -4.9990234375, -1.9990234375  # the frame's minimum in y and z, and row 0 holds its minimum in x
    pts[:, 1] = np.maximum(pts[:, 1], -4.9990234375)
    pts[:, 2] = np.maximum(pts[:, 2], -1.9990234375)
    mask = np.zeros(100, np.uint8)
    mask[[3, 7, 11, 20, 21, 22, 40, 41, 60, 61, 62, 80, 81, 90, 98, 99]] = 1  # neither row 0 nor row 50
    sel, cen, raw, st = sample_raw(pn2, cuda, pts, 16, 10, 10, mask=mask)
    wsel, wcen, wraw, _ = F.sample(pts, 16, 10, 10, mask=mask)
    assert st == 0 and np.array_equal(sel, wsel) and _same32(cen, wcen) and _same64(raw, wraw)
    assert np.allclose(cen.min(axis=0), [-5, -5, 0], atol=1e-6)
    by_frame_min = F.center(np.concatenate([pts[sel], pts[[0, 50]]]), 10, 10)[:16].astype(np.float32)
    assert not np.array_equal(cen[:, 0], by_frame_min[:, 0]) and not np.array_equal(cen[:, 1], by_frame_min[:, 1])
    assert not np.array_equal(cen[:, 2], by_frame_min[:, 2])


# ---- KittiFileData ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("ci", range(8))
def test_file_data_equals_the_golden(pn2, cuda, gold, ci):
    import torch
    tag = "c%d_" % ci
    n, cnt, bx, by, _ = (int(v) for v in gold[tag + "meta"])
    frame, mask = gold[tag + "frame"], gold[tag + "mask"]
    want_pts = frame[gold[tag + "source_index"], :3].astype(np.float64)
    dev_frame = torch.from_numpy(frame).to(cuda)
    for given in (frame, dev_frame, dev_frame[:, :3], frame[:, :3]):  # arrays and device tensors, 4 columns, 3 of 4, 3
        fd = pn2.dataset.KittiFileData(given, bx, by, device=cuda)
        assert len(fd) == cnt and fd.points.dtype == torch.float64 and fd.source_index.dtype == torch.int32
        assert _same64(fd.points.cpu().numpy(), want_pts)
        src = fd.source_index.cpu().numpy()
        assert np.array_equal(src, gold[tag + "source_index"])
        assert _same64(frame[src, :3].astype(np.float64), fd.points.cpu().numpy())
        assert tuple(fd.labels.shape) == (cnt,) and not bool(fd.labels.any())
        assert tuple(fd.colors.shape) == (cnt, 3) and fd.colors.dtype == torch.float64 and not bool(fd.colors.any())
    centered, raw = fd.get_batch_of_one_z_box_from_origin(n, sample_mask=mask if cnt > n else None)
    fd.check_last()
    assert centered.dtype == torch.float32 and raw.dtype == torch.float64 and centered.is_cuda and raw.is_cuda
    assert tuple(centered.shape) == (1, n, 3) == tuple(raw.shape)
    assert _same64(raw.cpu().numpy(), gold[tag + "raw"])
    assert _same32(centered.cpu().numpy(), gold[tag + "centered"].astype(np.float32))
    assert np.array_equal(fd.last_sel.cpu().numpy(), gold[tag + "sel"])
    if cnt > n:
        with pytest.raises(ValueError, match="sample_mask"):
            fd.get_batch_of_one_z_box_from_origin(n, sample_mask=mask[:-1])
        fd.get_batch_of_one_z_box_from_origin(n, sample_mask=np.ones(cnt, np.uint8))
        with pytest.raises(RuntimeError, match="status 3"):
            fd.check_last()


def test_file_data_empty_box_and_ties(pn2, cuda):
    far = np.full((100, 4), 50.0, dtype=np.float32)
    with pytest.raises(ValueError, match="no point of the frame lies in the box"):
        pn2.dataset.KittiFileData(far, 10, 10, device=cuda)
    with pytest.raises(ValueError, match="no point of the frame lies in the box"):
        pn2.dataset.KittiFileData(far[:0], 10, 10, device=cuda)
    with pytest.raises(ValueError, match="float32"):
        pn2.dataset.KittiFileData(far.astype(np.float64), 10, 10, device=cuda)
    frame = F.tie_frame()
    fd = pn2.dataset.KittiFileData(frame, 10, 10, device=cuda)
    pts, src = F.file_data(frame, 10, 10)
    assert np.array_equal(fd.source_index.cpu().numpy(), src) and _same64(fd.points.cpu().numpy(), pts)
    same = pts[1:, 0] == pts[:-1, 0]
    got = fd.source_index.cpu().numpy()
    assert same.sum() > 100 and np.all(got[1:][same] > got[:-1][same])  # rows with equal x stay in frame order


# ---- end to end ------------------------------------------------------------------------------------------------------------
def randomize_bn(store, seed):
    """non-trivial BN statistics so that folding is actually exercised"""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in store.params.items():
            if k.endswith("bn/gamma"):
                v.copy_((torch.rand(v.shape, generator=g) + 0.5).to(v.device))
            elif k.endswith("bn/beta") or k.endswith("biases"):
                v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(v.device))
        for k, v in store.buffers.items():
            if k.endswith("moving_mean"):
                v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(v.device))
            elif k.endswith("moving_variance"):
                v.copy_((torch.rand(v.shape, generator=g) + 0.5).to(v.device))
    store.train_epoch += 1  # the folded inference weights are made again from these values


def _lidar_frame(seed, n):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(-40, 40, n), rs.uniform(-15, 15, n), rs.uniform(-3, 6, n), rs.random_sample(n)], 1).astype(np.float32)


def _ground_frame(seed, n):
    """points dense enough around the 10 x 10 box for the balls of the SA levels to hold neighbours: a ground layer under the sensor"""
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(-8, 8, n), rs.uniform(-8, 8, n), -1.7 + np.abs(rs.normal(0, 0.3, n)), rs.random_sample(n)],
                    1).astype(np.float32)


def test_predict_and_interpolate_equals_the_eager_route(pn2, cuda):
    import torch
    hp = dict(pn2.model.SEMANTIC_NO_COLOR_HYPERPARAMS)
    hp.update(num_point=1024, l1_npoint=128, l2_npoint=64, l3_npoint=32, l4_npoint=16, box_size_x=10, box_size_y=10)
    pi = pn2.kitti_predict.PredictInterpolator(None, 9, hp, device=cuda)
    store = pi.predictor.store
    randomize_bn(store, 31)
    # fresh variables on colourless input predict one class everywhere (the part of the logits all points share decides); the
    # class biases are set so that every class's logit has mean zero over a frame, before anything is captured
    probe = pn2.dataset.KittiFileData(_ground_frame(1, 4000), 10, 10, device=cuda).get_batch_of_one_z_box_from_origin(1024)[0]
    pn2.util.tf_util.set_default_store(store)
    with torch.no_grad():
        store.params["fc2/biases"] -= pn2.model.get_model(probe, False, 9, hp)[0].mean(dim=(0, 1))
    store.train_epoch += 1
    for k, seed in enumerate((1, 2)):  # the first frame captures forward + argmax, the second replays the graph
        frame = _ground_frame(seed, 4000)
        fd = pn2.dataset.KittiFileData(frame, hp["box_size_x"], hp["box_size_y"], device=cuda, seed=seed)
        assert len(fd) > 1024 + 256  # the device draws a subset
        centered, raw = fd.get_batch_of_one_z_box_from_origin(1024)
        fd.check_last()
        labels, colors = pi.predict_and_interpolate(centered, raw, fd.points)
        assert labels.dtype == torch.int32 and tuple(labels.shape) == (len(fd),) and labels.is_cuda
        assert colors.dtype == torch.uint8 and tuple(colors.shape) == (len(fd), 3)
        pn2.util.tf_util.set_default_store(pi.predictor.store)
        with torch.no_grad():
            logits, _ = pn2.model.get_model(centered, False, 9, hp)
        torch.cuda.synchronize()
        sparse = torch.from_numpy(np.argmax(logits.cpu().numpy(), 2).astype(np.int32)).to(cuda)
        assert len(torch.unique(sparse)) > 1  # not a constant prediction
        want_l, want_c = pn2.interpolate_label_with_color(raw.to(torch.float32).reshape(-1, 3).contiguous(), sparse.reshape(-1),
                                                          fd.points.to(torch.float32).contiguous(), 3)
        assert torch.equal(labels, want_l) and torch.equal(colors, want_c), "frame %d" % k
        # numpy inputs, and a batch of two flattened as the reference's reshape([-1, 3]) does
        l2, _ = pi.predict_and_interpolate(centered.cpu().numpy(), raw.cpu().numpy(), fd.points.cpu().numpy())
        assert torch.equal(l2, labels)
        # back to the raw frame: -1 exactly on the rows the crop dropped
        full = pi.labels_for_raw_frame(fd, labels, len(frame)).cpu().numpy()
        _, kept = F.crop(frame, *F.kitti_box(hp["box_size_x"], hp["box_size_y"]))
        dropped = np.ones(len(frame), bool)
        dropped[kept] = False
        assert full.dtype == np.int32 and np.all(full[dropped] == -1) and np.all(full[kept] >= 0)
        assert np.array_equal(full[fd.source_index.cpu().numpy()], labels.cpu().numpy())
        # label_frame is the same route on a frame whose counter stands where fd's stood
        fresh = pn2.dataset.KittiFileData(frame, hp["box_size_x"], hp["box_size_y"], device=cuda, seed=seed)
        l3, c3 = pi.label_frame(fresh)
        assert torch.equal(l3, labels) and torch.equal(c3, colors)
    assert list(pi.predictor._graphs) == [(1, 1024)]
    # a batch of two is flattened to one sparse set, as the reference's reshape([-1, 3]) does
    raw2 = torch.cat([raw, raw + 0.25])
    centered2 = torch.cat([centered, centered.flip(1)])
    both = pi.predict_and_interpolate(centered2, raw2, fd.points)
    pn2.util.tf_util.set_default_store(pi.predictor.store)
    with torch.no_grad():
        logits2, _ = pn2.model.get_model(centered2, False, 9, hp)
    sparse2 = torch.from_numpy(np.argmax(logits2.cpu().numpy(), 2).astype(np.int32)).to(cuda)
    want2 = pn2.interpolate_label_with_color(raw2.to(torch.float32).reshape(-1, 3).contiguous(), sparse2.reshape(-1),
                                             fd.points.to(torch.float32).contiguous(), 3)
    assert torch.equal(both[0], want2[0]) and torch.equal(both[1], want2[1])


# ---- file route ------------------------------------------------------------------------------------------------------------
def test_dataset_reads_the_kitti_layout(pn2, cuda, tmp_path):
    folder = tmp_path / "2011_09_26" / "2011_09_26_drive_0095_sync" / "velodyne_points" / "data"
    folder.mkdir(parents=True)
    frames = [_lidar_frame(10 + k, 3000 + 500 * k) for k in range(3)]
    for k, fr in enumerate(frames):
        fr.tofile(str(folder / ("%010d.bin" % (k + 4))))
    ds = pn2.dataset.KittiDataset(1024, str(tmp_path), ["2011_09_26"], ["0095"], 60, 20, device=cuda)
    assert len(ds.list_file_data) == 3
    for k, fd in enumerate(ds.list_file_data):
        assert fd.file_path_without_ext == os.path.join("2011_09_26", "0095", "%04d" % k)
        pts, src = F.file_data(frames[k], 60, 20)
        assert _same64(fd.points.cpu().numpy(), pts) and np.array_equal(fd.source_index.cpu().numpy(), src)
        assert fd.num_frame_points == len(frames[k])
    assert _same64(ds.list_file_data[-1].points.cpu().numpy(), F.file_data(frames[2], 60, 20)[0])
    (folder / "0000000099.bin").write_bytes(b"\0" * 20)
    with pytest.raises(ValueError, match="rows of 4"):
        pn2.dataset.KittiDataset(1024, str(tmp_path), ["2011_09_26"], ["0095"], 60, 20, device=cuda).list_file_data[3]


def test_example_synthetic_file_route(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    root = tmp_path / "kitti"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "predict_kitti.py"), "--synthetic", "3", "4096", "--save", "--kitti_root",
           str(root)]
    run = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-3000:]
    assert out.count(" FPS] load_data: ") == 3 and out.count("Exported dense_labels to") == 3
    frames = pn2.dataset.kitti_dataset.list_frames(str(root), ["2011_09_26"], ["0095"])
    assert len(frames) == 3
    for k, (path, name) in enumerate(frames):
        frame = np.fromfile(path, dtype=np.float32).reshape(-1, 4)
        assert len(frame) == 4096 and name.endswith("%04d" % k)
        pts, _ = F.file_data(frame, 60, 20)
        assert len(pts) > 0
        labels = U.load_labels(str(tmp_path / "result" / "dense" / ("%04d.labels" % k)))
        dense, _ = U.read_point_cloud_pcd(str(tmp_path / "result" / "dense" / ("%04d.pcd" % k)))
        assert labels.shape == (len(pts),) and labels.min() >= 0 and labels.max() < 9
        assert dense.shape == (len(pts), 3) and np.array_equal(dense.astype(np.float32), pts.astype(np.float32))
