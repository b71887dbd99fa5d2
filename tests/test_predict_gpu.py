"""GPU tests of pn2.predict: Predictor (checkpoint -> captured forward + argmax per batch shape), predict_scene (per-scene
batches -> sparse points and labels, sparse confusion matrix), label_dense (chunked 3-NN vote + dense confusion matrix) and the
examples/predict_semantic3d.py file route."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import s_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiscene_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, N, C = 8, 2048, 9


def _hp(pn2):
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(num_point=N, l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16)
    return hp


def _cloud(cuda, seed, b=B, n=N, colour=True):
    import torch
    rs = np.random.RandomState(seed)
    parts = [s_scene(seed + 1, b, n)] + ([rs.random_sample((b, n, 3)).astype(np.float32)] if colour else [])
    return torch.from_numpy(np.concatenate(parts, 2)).to(cuda)


def _eager(pn2, predictor, pc):
    """np.argmax of an eager inference forward under the predictor's store"""
    import torch
    pn2.util.tf_util.set_default_store(predictor.store)
    with torch.no_grad():
        logits, _ = pn2.model.get_model(pc, False, predictor.num_classes, predictor.hp)
    torch.cuda.synchronize()
    return np.argmax(logits.cpu().numpy(), 2).astype(np.int32)


@pytest.fixture(scope="module")
def predictor(pn2, cuda):
    return pn2.predict.Predictor(None, C, _hp(pn2), device=cuda, seed=5)


def test_predict_equals_eager_argmax_on_capture_and_replays(pn2, cuda, predictor):
    import torch
    a, b = _cloud(cuda, 1), _cloud(cuda, 2)
    first = predictor.predict(a)  # captures
    assert first.dtype == torch.int32 and tuple(first.shape) == (B, N) and first.is_cuda
    want_a = _eager(pn2, predictor, a)
    assert np.array_equal(first.cpu().numpy(), want_a)
    assert 1 < len(np.unique(want_a))  # not a constant prediction
    second = predictor.predict(b)  # a replay with other data
    assert np.array_equal(second.cpu().numpy(), _eager(pn2, predictor, b))
    assert np.array_equal(first.cpu().numpy(), want_a)  # the earlier result is the caller's: not overwritten
    assert first.data_ptr() != second.data_ptr()
    assert np.array_equal(predictor.predict(a.cpu().numpy()).cpu().numpy(), want_a)  # a numpy batch
    with pytest.raises(ValueError, match="use_color"):
        predictor.predict(a[:, :, :3])
    with pytest.raises(ValueError):
        predictor.predict(a[0])


def test_predict_leaves_the_default_store_alone(pn2, cuda, predictor):
    tfu = pn2.util.tf_util
    mine = tfu.set_default_store(tfu.VariableStore(device=cuda, seed=1))
    predictor.predict(_cloud(cuda, 6))
    assert tfu.get_default_store() is mine
    with pytest.raises(ValueError):
        predictor.predict(_cloud(cuda, 6)[:, :, :3])
    assert tfu.get_default_store() is mine and not mine.params


def test_batch_sizes_keep_their_graphs(pn2, cuda, predictor):
    full, part, again = _cloud(cuda, 3), _cloud(cuda, 4, b=3), _cloud(cuda, 5)
    for pc in (full, part, again):
        assert np.array_equal(predictor.predict(pc).cpu().numpy(), _eager(pn2, predictor, pc)), tuple(pc.shape)
    assert {(B, N), (3, N)} <= set(predictor._graphs)
    g8 = predictor._graphs[(B, N)][0]
    predictor.predict(part)
    predictor.predict(full)
    assert predictor._graphs[(B, N)][0] is g8  # the smaller batch did not evict the full-size graph


def test_checkpoint_of_a_trainer(pn2, cuda, tmp_path):
    import torch
    hp = _hp(pn2)
    tr = pn2.train.Trainer(hp, C, store=pn2.util.tf_util.VariableStore(device=cuda, seed=3), capture=False)
    rs = np.random.RandomState(0)
    for s in range(2):
        labels = torch.from_numpy(rs.randint(0, C, (B, N)).astype(np.int64)).to(cuda)
        w = torch.from_numpy((rs.random_sample((B, N)) + 0.5).astype(np.float32)).to(cuda)
        tr.train_step(_cloud(cuda, 10 + s), labels, w)
    path = str(tmp_path / "model.pt")
    tr.save(path)
    pc = _cloud(cuda, 20)
    tr.eval_step(pc, labels, w)
    torch.cuda.synchronize()
    want = np.argmax(tr.last_eval_logits.cpu().numpy(), 2).astype(np.int32)
    p = pn2.predict.Predictor(path, C, hp, device=cuda)
    got = p.predict(pc).cpu().numpy()
    assert np.array_equal(got, want)
    fresh = pn2.predict.Predictor(None, C, hp, device=cuda)
    assert not np.array_equal(fresh.predict(pc).cpu().numpy(), want)  # the checkpoint, not the initial values, decided
    with pytest.raises(ValueError, match="fc2/"):
        pn2.predict.Predictor(path, C + 1, hp, device=cuda)
    torch.save({"variables": {"nothing/weights": torch.zeros(3)}}, str(tmp_path / "other.pt"))
    with pytest.raises(ValueError, match="nothing/weights"):
        pn2.predict.Predictor(str(tmp_path / "other.pt"), C, hp, device=cuda)


SCENES = [(51, 30000, 20.0, 18.0), (52, 20000, 40.0, 30.0)]


def _dataset(pn2, cuda, seed):
    scenes = [R.synthetic_scene(*s) + ("scene%d" % i,) for i, s in enumerate(SCENES)]
    return pn2.dataset.SemanticDataset(N, "validation", True, 10, 10, "", device=cuda, seed=seed, scenes=scenes)


def _dataset_at(pn2, cuda, seed, counter, b):
    """the batch of size b of scene 0 (the dense one: columns wider than N) that a fresh same-seed dataset, which only ever uses that b, draws at batch counter `counter`"""
    ds = _dataset(pn2, cuda, seed)
    for _ in range(counter + 1):
        out = ds.sample_batch_in_file(0, b)
    ds.check_last()
    return out


def test_predict_scene_equals_the_hand_written_loop(pn2, cuda, predictor):
    import torch
    a, b = _dataset(pn2, cuda, 13), _dataset(pn2, cuda, 13)
    cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
    points, labels = pn2.predict.predict_scene(predictor, a, 1, 11, batch_size=4, confusion=cm)
    a.check_last()
    assert tuple(points.shape) == (11 * N, 3) and points.dtype == torch.float32
    assert tuple(labels.shape) == (11 * N,) and labels.dtype == torch.int32
    pts, lab, gts = [], [], []
    for bs in (4, 4, 3):
        data, raw, gt = b.sample_batch_in_file(1, bs)
        assert tuple(data.shape) == (bs, N, 6)
        pts.append(raw.reshape(-1, 3).float())
        lab.append(predictor.predict(data).reshape(-1))
        gts.append(gt.reshape(-1))
    assert torch.equal(points, torch.cat(pts)) and torch.equal(labels, torch.cat(lab))
    assert int(a.batch_counter.item()) == 3 == int(b.batch_counter.item())
    g, p = torch.cat(gts).cpu().numpy().astype(np.int64), torch.cat(lab).cpu().numpy().astype(np.int64)
    assert np.array_equal(cm.confusion_matrix.reshape(-1), np.bincount(g * C + p, minlength=C * C))
    assert cm.confusion_matrix.sum() == 11 * N
    # further scenes on the same dataset, the batch size growing again after each short last batch (4, 1 | 4, 1 | 4, 1), the
    # dense scene first and last: every sample is accepted, and the batches are those of datasets that only ever use one size
    for scene in (0, 1, 0):
        points2, labels2 = pn2.predict.predict_scene(predictor, a, scene, 5, batch_size=4)
        assert tuple(a.last_status.shape) == (1,)
        a.check_last()  # the worst status of all the scene's batches
    assert int(a.batch_counter.item()) == 9
    # predict_scene's last two calls were batch counters 7 (b = 4) and 8 (b = 1), both of scene 0
    (d4, r4, _), (d1, r1, _) = _dataset_at(pn2, cuda, 13, 7, 4), _dataset_at(pn2, cuda, 13, 8, 1)
    assert torch.equal(points2[:4 * N], r4.reshape(-1, 3).float()) and torch.equal(points2[4 * N:], r1.reshape(-1, 3).float())
    assert torch.equal(labels2[:4 * N], predictor.predict(d4).reshape(-1)) and torch.equal(labels2[4 * N:], predictor.predict(d1).reshape(-1))
    # without a matrix nothing is counted, and fewer samples than one batch give one small batch
    points1, labels1 = pn2.predict.predict_scene(predictor, a, 0, 2, batch_size=4)
    assert tuple(points1.shape) == (2 * N, 3) and int(a.batch_counter.item()) == 10
    with pytest.raises(ValueError):
        pn2.predict.predict_scene(predictor, a, 0, 0)


def test_label_dense_does_not_depend_on_the_chunk(pn2, cuda, predictor):
    import torch
    rs = np.random.RandomState(6)
    ns, nd = 20000, 200000
    sp_h = (rs.uniform(0, 20, (ns, 3)) * [1, 1, 0.2]).astype(np.float32)
    dp_h = (rs.uniform(0, 20, (nd, 3)) * [1, 1, 0.2]).astype(np.float32)
    sl_h = rs.randint(1, C, ns).astype(np.int32)
    gt_h = rs.randint(0, C, nd).astype(np.int32)
    sp, sl, dp, gt = (torch.from_numpy(x).to(cuda) for x in (sp_h, sl_h, dp_h, gt_h))
    want_l, want_c = pn2.interpolate_label_with_color(sp, sl, dp, 3)
    g, p = gt_h.astype(np.int64), want_l.cpu().numpy().astype(np.int64)
    want_cm = np.bincount(g * C + p, minlength=C * C)
    for kw, dense, truth in ((dict(chunk=4096), dp, gt), (dict(chunk=1 << 24), dp, gt), (dict(chunk=65536), dp_h, gt_h), ({}, dp, gt)):
        cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
        lab, col = pn2.predict.label_dense(sp, sl, dense, truth, confusion=cm, **kw)
        assert lab.dtype == torch.int32 and col.dtype == torch.uint8 and tuple(col.shape) == (nd, 3)
        assert torch.equal(lab, want_l) and torch.equal(col, want_c), kw
        assert np.array_equal(cm.confusion_matrix.reshape(-1), want_cm), kw
    # int64 ground truth is counted at 64 bits: 2^32 + class is dropped, not wrapped into a class
    wide = gt.long()
    wide[::3] += 1 << 32
    keep = np.ones(nd, bool)
    keep[::3] = False
    for truth in (wide, wide.cpu().numpy()):
        cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
        pn2.predict.label_dense(sp, sl, dp, truth, confusion=cm, chunk=70000)
        assert np.array_equal(cm.confusion_matrix.reshape(-1), np.bincount(g[keep] * C + p[keep], minlength=C * C))
    # without ground truth nothing is counted
    cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
    lab, _ = pn2.predict.label_dense(sp, sl, dp, None, confusion=cm, chunk=50000)
    assert torch.equal(lab, want_l) and not cm.confusion_matrix.any()
    lab, _ = pn2.predict.label_dense(sp_h, sl_h, dp, gt)  # numpy sparse side, ground truth without a matrix
    assert torch.equal(lab, want_l)
    # Predictor.interpolate_labels is the same vote with knn = 3
    lab, col = predictor.interpolate_labels(sp_h, sl_h, dp_h)
    assert torch.equal(lab, want_l) and torch.equal(col, want_c)


@pytest.mark.timeout(300)
def test_example_file_route_agrees_with_the_in_memory_route(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    scene_points, samples = 60000, 5
    cmd = [sys.executable, os.path.join(ROOT, "examples", "predict_semantic3d.py"), "--num_samples", str(samples), "--batch-size", "4",
           "--points", str(N), "--npoint", "256,64,32,16", "--scenes", "2", "--scene-points", str(scene_points), "--voxel", "0.1",
           "--chunk", "25000"]
    run = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-3000:]
    assert "Sparse results" in out and "Global results" in out and out.count("Confusion matrix:") == 4
    for k in range(2):
        name = "syn_validation_%d" % k
        sparse, dense = tmp_path / "result" / "sparse", tmp_path / "result" / "dense"
        sp, _ = U.read_point_cloud_pcd(str(sparse / (name + ".pcd")))
        sl = U.load_labels(str(sparse / (name + ".labels")))
        assert sp.shape == (samples * N, 3) and sl.shape == (samples * N,)
        assert sl.min() >= 0 and sl.max() < C
        dp, dc = U.read_point_cloud_pcd(str(dense / (name + "_colored.pcd")))
        dl = U.load_labels(str(dense / (name + ".labels")))
        assert dp.shape == (scene_points, 3) and dl.shape == (scene_points,)
        lab, col = pn2.predict.label_dense(sp.astype(np.float32), sl, dp.astype(np.float32))
        assert np.array_equal(lab.cpu().numpy(), dl)
        assert np.array_equal(col.cpu().numpy(), np.rint(dc * 255.0).astype(np.uint8))
