"""GPU tests of SemanticDataset.sample_batch_in_file (dataset/multi_scene.py): per-scene batches from the resident multi-scene
store -- the reference's list_file_data[i].sample_batch as predict.py:163 calls it -- checked against the numpy restatement
of the column crop and centring in tests/multiscene_ref.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiscene_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N, BOX, B = 2048, 10.0, 5
# (seed, points, x extent, y extent): ~83 points per m^2 -- a 10 m x 10 m column holds ~8000 > N points; ~17 per m^2 -- about
# 1700 < N; and a small scene in between
SCENES = [(41, 30000, 20.0, 18.0), (42, 20000, 40.0, 30.0), (43, 12000, 20.0, 15.0)]


def _scenes():
    return [R.synthetic_scene(*s) + ("scene%d" % i,) for i, s in enumerate(SCENES)]


def _dataset(pn2, cuda, seed=7):
    return pn2.dataset.SemanticDataset(N, "validation", True, BOX, BOX, "", device=cuda, seed=seed, scenes=_scenes())


@pytest.fixture(scope="module")
def batches(pn2, cuda):
    """one B = 5 batch per scene from one dataset, read back once: scene -> dict of numpy arrays"""
    ds = _dataset(pn2, cuda)
    out = {}
    for k in range(ds.num_scenes):
        before = int(ds.batch_counter.item())
        data, raw, lab = ds.sample_batch_in_file(k, B)
        ds.check_last()
        assert int(ds.batch_counter.item()) == before + 1
        assert data.dtype.is_floating_point and tuple(data.shape) == (B, N, 6) and data.is_contiguous()
        assert str(raw.dtype) == "torch.float64" and tuple(raw.shape) == (B, N, 3)
        assert str(lab.dtype) == "torch.int32" and tuple(lab.shape) == (B, N)
        out[k] = dict(data=data.cpu().numpy(), raw=raw.cpu().numpy(), lab=lab.cpu().numpy(),
                      scene=ds.last_scene.cpu().numpy(), center=ds.last_center.cpu().numpy(), cnt=ds.last_cnt.cpu().numpy(),
                      sel=ds.last_sel.cpu().numpy())
    return ds, out


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_batch_comes_from_the_scene_and_matches_the_reference_centring(batches, k):
    ds, out = batches
    o = out[k]
    lo, hi = int(ds.scene_offsets[k]), int(ds.scene_offsets[k + 1])
    store_p = np.concatenate(ds.scene_points)
    store_l = np.concatenate(ds.scene_labels)
    store_c = np.concatenate(ds.scene_colors)
    assert o["data"].dtype == np.float32
    assert np.array_equal(o["scene"], np.full(B, k))
    assert o["sel"].min() >= lo and o["sel"].max() < hi
    assert np.array_equal(o["raw"], store_p[o["sel"]])
    assert np.array_equal(o["lab"], store_l[o["sel"]])
    pts = ds.scene_points[k]
    for s in range(B):
        assert 0 <= o["center"][s] < len(pts)
        members = lo + np.nonzero(R.column(pts, pts[o["center"][s]], BOX / 2, BOX / 2))[0]
        assert o["cnt"][s] == len(members)
        assert np.isin(o["sel"][s], members).all()  # every selected point lies in the column of its centre
        if len(members) > N:
            assert (np.diff(o["sel"][s]) > 0).all()  # N distinct ascending indices
        else:
            assert np.array_equal(o["sel"][s], members[np.arange(N) % len(members)])  # the index list repeated
        want = R.center_box(store_p[o["sel"][s]], BOX / 2, BOX / 2).astype(np.float32)  # float64 centring, then float32
        assert np.array_equal(o["data"][s, :, :3], want)
        assert np.array_equal(o["data"][s, :, 3:], store_c[o["sel"][s]].astype(np.float32))


def test_the_scenes_cover_both_column_kinds(batches):
    """the dense scene's columns exceed N, the sparse scene's do not: both branches of the subset step ran"""
    _, out = batches
    print("column sizes per scene:", {k: sorted(o["cnt"].tolist()) for k, o in out.items()})
    assert (out[0]["cnt"] > N).any()
    assert (out[1]["cnt"] <= N).all()


def test_same_seed_same_sequence_same_batches(pn2, cuda):
    import torch
    a, b = _dataset(pn2, cuda, seed=9), _dataset(pn2, cuda, seed=9)
    seen = []
    for step, k in enumerate([2, None, 0, 1, None, 1]):  # None: a sample_batch_in_all_files call in between
        before = int(a.batch_counter.item())
        if k is None:
            x, y = a.sample_batch_in_all_files(3, augment=True), b.sample_batch_in_all_files(3, augment=True)
        else:
            x, y = a.sample_batch_in_file(k, 3), b.sample_batch_in_file(k, 3)
            seen.append((k, x[0]))
        for u, v in zip(x, y):
            assert torch.equal(u, v), step
        assert torch.equal(a.last_sel, b.last_sel) and torch.equal(a.last_scene, b.last_scene)
        assert int(a.batch_counter.item()) == before + 1 and int(b.batch_counter.item()) == before + 1
    a.check_last()
    # two calls for one scene draw different batches (the counter moved)
    assert not torch.equal(seen[2][1], seen[3][1]) and seen[2][0] == seen[3][0] == 1


def test_scene_index_out_of_range(pn2, cuda):
    ds = _dataset(pn2, cuda)
    for bad in (-1, ds.num_scenes):
        with pytest.raises(ValueError, match="scene"):
            ds.sample_batch_in_file(bad, 2)
    with pytest.raises(ValueError):
        ds.sample_batch_in_file(0, 0)


def test_batch_size_may_shrink_and_grow_again(pn2, cuda):
    """b = 4, then b = 1, then b = 4 on ONE dataset, on the dense scene (columns wider than N: the candidate lists are written):
    every batch equals the batch of a same-seed dataset that only ever uses that b -- the draws depend on (seed, batch counter,
    sample), not on b -- and no sample is rejected.  (Workspaces are laid out by b: one shared between batch sizes hands the
    larger b a smaller one's candidate lists where its histogram must be zero.)  The multi-scene call shares the workspaces."""
    import torch
    mixed, only4, only1 = (_dataset(pn2, cuda, seed=21) for _ in range(3))
    wide = {1: False, 4: False}
    for step, b in enumerate([4, 1, 4, 1, 4]):
        got = mixed.sample_batch_in_file(0, b)
        mixed.check_last()
        wide[b] = wide[b] or bool((mixed.last_cnt > N).any())
        for other, ob in ((only4, 4), (only1, 1)):
            want = other.sample_batch_in_file(0, ob)
            other.check_last()
            if ob == b:
                for u, v in zip(got, want):
                    assert torch.equal(u, v), step
                assert torch.equal(mixed.last_sel, other.last_sel), step
    assert wide[1] and wide[4]  # both batch sizes met columns wider than N: their candidate lists were written
    for step, b in enumerate([2, 5, 2, 5]):  # sample_batch_in_all_files after sample_batch_in_file, growing and shrinking
        got = mixed.sample_batch_in_all_files(b, augment=False)
        mixed.check_last()
        for other, ob in ((only4, 5), (only1, 2)):
            want = other.sample_batch_in_all_files(ob, augment=False)
            other.check_last()
            if ob == b:
                for u, v in zip(got, want):
                    assert torch.equal(u, v), step
