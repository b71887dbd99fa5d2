"""CPU tests of pn2.dataset.SemanticDataset: the numpy restatement against the fixture frozen from the reference's own code
(tests/golden/make_multiscene_golden.py), the scene-pick rule the kernel implements, the host attributes, file loading and
argument validation of the new entry points -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiscene_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "multiscene_sampler.npz")
NCASES = 5


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _case(pn2, g, ci):
    b, n, box, use_color, augment, seed = [int(v) for v in g["c%d_meta" % ci]]
    split = str(g["c%d_split" % ci])
    names = list(g["splits_" + split])
    scenes = [s for s in R.synthetic_scenes() if s[3] in names]
    ds = pn2.dataset.SemanticDataset(n, split, bool(use_color), box, box, "data", device="cpu", scenes=scenes)
    return ds, b, bool(augment), seed


@pytest.mark.parametrize("ci", range(NCASES))
def test_restatement_reproduces_the_fixture(pn2, gold, ci):
    ds, b, augment, seed = _case(pn2, gold, ci)
    np.random.seed(seed)
    rec = R.Recorder()
    data, lab, wts = R.sample_batch(R.HostDataset(ds), b, augment, rec)
    t = "c%d_" % ci
    assert str(data.dtype) == str(gold[t + "data_dtype"]) and str(wts.dtype) == str(gold[t + "weights_dtype"])
    assert np.array_equal(data, gold[t + "data"])
    assert np.array_equal(lab, gold[t + "label"]) and np.array_equal(wts, gold[t + "weights"])
    d = rec.draws(b)
    for k in ("scene", "center", "masks", "angle"):
        assert np.array_equal(d[k], gold[t + "draw_" + k]), k


def test_fixture_covers_the_cases(gold):
    metas = [gold["c%d_meta" % i] for i in range(NCASES)]
    assert {int(m[3]) for m in metas} == {0, 1} and {int(m[4]) for m in metas} == {0, 1}
    assert {str(gold["c%d_split" % i]) for i in range(NCASES)} == {"train", "validation"}
    cnt = np.concatenate([gold["c%d_cnt" % i] for i in range(NCASES)])
    npts = np.concatenate([[int(m[1])] * int(m[0]) for m in metas])
    assert (cnt > npts).any() and (cnt <= npts).any()
    assert any(len(set(gold["c%d_draw_scene" % i].tolist())) < len(gold["c%d_draw_scene" % i]) for i in range(NCASES))


def test_choice_is_the_cdf_searchsorted_rule():
    """np.random.choice(k, p) == cdf.searchsorted(random_sample(), side='right') with cdf = p.cumsum() / last: the rule
    ds_count implements (a uniform double against the float64 CDF)."""
    rs = np.random.RandomState(0)
    for trial in range(20):
        k = rs.randint(1, 12)
        p = rs.randint(1, 10 ** 6, k).astype(np.float64)
        p = p / p.sum()
        cdf = p.cumsum()
        cdf /= cdf[-1]
        for s in range(100):
            a = np.random.RandomState(1000 * trial + s).choice(k, p=p)
            u = np.random.RandomState(1000 * trial + s).random_sample()
            assert a == int(cdf.searchsorted(u, side="right"))


@pytest.mark.parametrize("ci", range(NCASES))
def test_host_attributes_match_the_fixture(pn2, gold, ci):
    ds, b, _, _ = _case(pn2, gold, ci)
    t = "c%d_" % ci
    assert ds.scene_probas.dtype == np.float64 and np.array_equal(ds.scene_probas, gold[t + "scene_probas"])
    lw = gold[t + "label_weights"]
    assert ds.label_weights.dtype == lw.dtype and np.array_equal(ds.label_weights, lw)
    if ds.split == "train":
        assert lw.dtype == np.float32 and (lw > 0).all()
    else:
        assert not lw.any()
    assert ds.get_total_num_points() == int(gold[t + "total"])
    assert [ds.get_num_batches(k) for k in (1, 2, 4, 16)] == gold[t + "num_batches"].tolist()
    assert ds.num_classes == 9 and len(ds.labels_names) == 9 and ds.num_scenes == len(ds.scene_points)


def test_label_weights_close_the_last_bin(pn2):
    """np.histogram(labels, range(10)) closes its last bin: a label 9 counts with 8"""
    labels = [np.array([0, 1, 8, 9, 9], dtype=np.int32)]
    w = pn2.dataset.multi_scene.label_weights_of(labels)
    freq = np.array([1, 1, 0, 0, 0, 0, 0, 0, 3], dtype=np.float32) / np.float32(5)
    assert w.dtype == np.float32 and np.array_equal(w, 1 / np.log(1.2 + freq))


def test_default_split_table(pn2):
    t = pn2.dataset.multi_scene.default_splits()
    assert len(t["train"]) == 9 and len(t["validation"]) == 6 and len(t["test"]) == 15
    assert t["train_full"] == t["train"] + t["validation"]
    assert t["all"] == t["train"] + t["validation"] + t["test"]
    assert len(set(t["all"])) == 30 and "bildstein_station1_xyz_intensity_rgb" == t["train"][0]


def test_files_load_like_arrays(pn2, tmp_path):
    wp = pn2.util.point_cloud_util
    scenes = R.synthetic_scenes()[:3]
    for p, l, c, name in scenes:
        wp.write_point_cloud_pcd(str(tmp_path / (name + ".pcd")), p, c)
        wp.write_labels(str(tmp_path / (name + ".labels")), l)
    splits = {"train": [s[3] for s in scenes], "test": [s[3] for s in scenes[:2]]}
    a = pn2.dataset.SemanticDataset(256, "train", True, 4, 4, str(tmp_path), device="cpu", splits=splits)
    # what the reader gives: float32 coordinates, colours quantised to 1/255 steps
    loaded = [(wp.read_point_cloud_pcd(str(tmp_path / (s[3] + ".pcd")))[0], s[1],
               wp.read_point_cloud_pcd(str(tmp_path / (s[3] + ".pcd")))[1], s[3]) for s in scenes]
    b = pn2.dataset.SemanticDataset(256, "train", True, 4, 4, str(tmp_path), device="cpu", scenes=loaded)
    for x, y in zip(a.scene_points + a.scene_labels + a.scene_colors, b.scene_points + b.scene_labels + b.scene_colors):
        assert np.array_equal(x, y)
    assert np.array_equal(a.label_weights, b.label_weights) and np.array_equal(a.scene_probas, b.scene_probas)
    assert a.get_file_paths_without_ext() == [os.path.join(str(tmp_path), s[3]) for s in scenes]
    t = pn2.dataset.SemanticDataset(256, "test", False, 4, 4, str(tmp_path), device="cpu", splits=splits)  # no .labels read
    assert t.num_scenes == 2 and not any(l.any() for l in t.scene_labels) and not t.label_weights.any()
    with pytest.raises(ValueError):
        pn2.dataset.SemanticDataset(256, "nope", True, 4, 4, str(tmp_path), device="cpu", splits=splits)


def test_argument_validation_needs_no_gpu(pn2):
    import ctypes
    L = pn2._lib.lib
    nul = None
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    v = ctypes.c_ulonglong(0)
    assert L.pn2_dataset_workspace_size(0, 4, ctypes.c_void_p(ctypes.addressof(v))) == -1
    assert L.pn2_dataset_workspace_size(2, 4, nul) == -2
    assert L.pn2_dataset_workspace_size(2, 4, ctypes.c_void_p(ctypes.addressof(v))) == 0 and v.value > 0

    def call(**kw):
        a = dict(b=2, npts=64, ns=1, mc=4, color=1, aug=1, pts=fake, col=nul, lab=nul, off=fake, cdf=fake, zs=fake, lw=nul,
                 nlw=0, hx=2.0, hy=2.0, seed=0, ctr=fake, dsc=nul, dce=nul, dma=nul, cap=0, drot=nul, ws=fake,
                 wsb=v.value, info=fake, finfo=fake, sel=fake, data=fake, olab=fake, ow=fake, stream=nul)
        a.update(kw)
        return L.pn2_dataset_sample(*a.values())
    assert call(b=0) == -1 and call(npts=0) == -1 and call(ns=0) == -1 and call(mc=0) == -1
    assert call(hx=0.0) == -1                                 # box sizes > 0
    assert call(pts=nul) == -2 and call(ws=nul) == -2 and call(data=nul) == -2
    assert call(ctr=nul) == -2                                # device draws need the batch counter
    assert call(nlw=9) == -2                                  # weights announced, none given
    assert call(dsc=fake) == -1                               # replay needs the centres ...
    assert call(dsc=fake, dce=fake) == -1                     # ... and the angles when augmenting
    assert call(dce=fake) == -1                               # draws are all given or none
    assert call(wsb=v.value - 1) == -1                        # workspace too small
    ds = pn2.dataset.SemanticDataset(64, "train", True, 4, 4, "", device="cpu", scenes=R.synthetic_scenes()[:1])
    with pytest.raises(ValueError):
        pn2.dataset.SemanticDataset(0, "train", True, 4, 4, "", device="cpu", scenes=R.synthetic_scenes()[:1])
    with pytest.raises(ValueError):
        ds.sample_batch_in_all_files(0)
