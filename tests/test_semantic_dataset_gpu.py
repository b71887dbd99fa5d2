"""GPU tests of pn2.dataset.SemanticDataset (csrc/pn2_dataset.hip): replay parity with the reference's batches, validity of
the device-random batches at full size, determinism and graph capture, the sampling distributions, and the batches
feeding Trainer.train_step / eval_step."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiscene_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "multiscene_sampler.npz")
NCASES = 5


def _ulps(a, b):
    """distance in float32 ulps (same-sign values; both arrays float32)"""
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("ci", range(NCASES))
def test_replay_parity_with_the_reference(pn2, cuda, ci):
    g = np.load(GOLD)
    t = "c%d_" % ci
    b, n, box, use_color, augment, _ = [int(v) for v in g[t + "meta"]]
    split = str(g[t + "split"])
    names = list(g["splits_" + split])
    ds = pn2.dataset.SemanticDataset(n, split, bool(use_color), box, box, "", device=cuda,
                                     scenes=[s for s in R.synthetic_scenes() if s[3] in names])
    draws = {k: g[t + "draw_" + k] for k in ("scene", "center", "masks", "angle")}
    data, lab, wts = ds.sample_batch_in_all_files(b, augment=bool(augment), draws=draws)
    ds.check_last()
    data, lab, wts = data.cpu().numpy(), lab.cpu().numpy(), wts.cpu().numpy()
    assert data.shape == (b, n, 6 if use_color else 3) and lab.dtype == np.int32 and wts.dtype == np.float32
    assert np.array_equal(ds.last_cnt.cpu().numpy(), g[t + "cnt"])
    assert np.array_equal(lab, g[t + "label"])
    assert np.array_equal(wts, g[t + "weights"].astype(np.float32))
    want = g[t + "data"].astype(np.float32)  # un-augmented: the reference's float64 batch, fed as float32
    if use_color:
        assert np.array_equal(data[:, :, 3:], want[:, :, 3:])
    if not augment:
        assert np.array_equal(data, want)
    else:
        u = _ulps(data[:, :, :3], want[:, :, :3])
        off = int((u > 0).sum())
        print("case %d: %d of %d rotated values differ by 1 ulp (numpy BLAS rounding of p @ R)" % (ci, off, u.size))
        assert u.max() <= 1 and off <= 1e-4 * u.size + 1  # 0.01 %, at least one value allowed at these small sizes


def _fullsize_scenes():
    """three scenes dense enough that a 10 m x 10 m column away from the edges holds 50k+ points"""
    spec = [(21, 1500000, 60.0, 40.0), (22, 800000, 40.0, 30.0), (23, 500000, 30.0, 30.0)]
    return [R.synthetic_scene(*s) + ("big%d" % i,) for i, s in enumerate(spec)]


@pytest.fixture(scope="module")
def big(pn2, cuda):
    return pn2.dataset.SemanticDataset(8192, "train", True, 10, 10, "", device=cuda, seed=5, scenes=_fullsize_scenes())


def test_device_random_batches_are_valid_at_full_size(pn2, cuda, big):
    ds = big
    B, N = 16, 8192
    data, lab, wts = ds.sample_batch_in_all_files(B, augment=True)
    ds.check_last()
    data, lab, wts = data.cpu().numpy(), lab.cpu().numpy(), wts.cpu().numpy()
    scene, center, cnt = ds.last_scene.cpu().numpy(), ds.last_center.cpu().numpy(), ds.last_cnt.cpu().numpy()
    sel, angle = ds.last_sel.cpu().numpy(), ds.last_angle.cpu().numpy()
    print("column sizes:", sorted(cnt.tolist()))
    assert np.median(cnt) >= 50000
    store_p = np.concatenate(ds.scene_points)
    store_l = np.concatenate(ds.scene_labels)
    store_c = np.concatenate(ds.scene_colors).astype(np.float32)
    worst = 0
    for s in range(B):
        k, o = int(scene[s]), int(ds.scene_offsets[scene[s]])
        pts = ds.scene_points[k]
        members = o + np.nonzero(R.column(pts, pts[center[s]], 5.0, 5.0))[0]
        assert cnt[s] == len(members)
        m = min(N, len(members))
        head = sel[s, :m]
        assert (np.diff(head) > 0).all() and np.isin(head, members).all()
        if len(members) <= N:
            assert np.array_equal(head, members) and np.array_equal(sel[s], members[np.arange(N) % len(members)])
        want = R.center_box(store_p[sel[s]], 5.0, 5.0) @ R.rotation(angle[s])
        u = _ulps(data[s, :, :3], want.astype(np.float32))
        worst = max(worst, int(u.max()))
        assert u.max() <= 1
        assert np.array_equal(data[s, :, 3:], store_c[sel[s]])
        assert np.array_equal(lab[s], store_l[sel[s]])
        assert np.array_equal(wts[s], ds.label_weights[store_l[sel[s]]])
    assert 0.0 <= angle.min() and angle.max() < 2 * np.pi
    print("worst rotated-xyz distance: %d ulp" % worst)


def test_same_seed_same_batches_and_capture_replays_fresh_ones(pn2, cuda):
    import torch
    scenes = R.synthetic_scenes()
    mk = lambda: pn2.dataset.SemanticDataset(256, "train", True, 4, 4, "", device=cuda, seed=9, scenes=scenes)  # noqa: E731
    a, b = mk(), mk()
    x1, x2 = a.sample_batch_in_all_files(8), b.sample_batch_in_all_files(8)
    for u, v in zip(x1, x2):
        assert torch.equal(u, v)
    y1 = a.sample_batch_in_all_files(8)
    assert not torch.equal(x1[0], y1[0])  # consecutive calls differ
    b.sample_batch_in_all_files(8)  # both datasets are now at batch counter 2
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            out = a.sample_batch_in_all_files(8)
    torch.cuda.current_stream().wait_stream(s)
    assert int(a.batch_counter.item()) == 2  # capture launches nothing
    for k in range(4):
        g.replay()
        got = [t.clone() for t in out]
        want = b.sample_batch_in_all_files(8)
        for u, v in zip(got, want):
            assert torch.equal(u, v), k
        if k:
            assert not torch.equal(got[0], prev)
        prev = got[0]
    torch.cuda.synchronize()
    assert int(a.batch_counter.item()) == 6 and int(b.batch_counter.item()) == 6


def test_sampling_distributions(pn2, cuda):
    """Fixed seeds: the statistics below are deterministic, and each bound is a 99.9 % quantile of the statistic's null
    distribution, so a correct sampler passes with probability 0.999 for a seed drawn at random.
      * scene frequencies over 4096 samples: Pearson's X^2 against scene_probas, df = scenes - 1 -> chi2.ppf(0.999, df);
      * angles over the same samples: Kolmogorov-Smirnov D against U[0, 2 pi): sqrt(n) D < 1.949 (Kolmogorov 0.999);
      * member hit counts for a scene smaller than one column (every sample is the whole scene, cnt = 2000, N = 256) over
        4096 samples: X^2 = sum (h - e)^2 / e, e = 4096 N / cnt.  Without replacement inside a sample the variance of a
        count is e (1 - N/cnt) < e, so X^2 is stochastically below chi2(cnt - 1): its 99.9 % quantile is a safe bound."""
    import torch
    from scipy import stats
    scenes = R.synthetic_scenes()
    ds = pn2.dataset.SemanticDataset(256, "train", True, 4, 4, "", device=cuda, seed=17, scenes=scenes)
    sc, an = [], []
    for _ in range(64):
        ds.sample_batch_in_all_files(64)
        sc.append(ds.last_scene.clone())
        an.append(ds.last_angle.clone())
    ds.check_last()
    sc = torch.cat(sc).cpu().numpy()
    an = torch.cat(an).cpu().numpy()
    obs = np.bincount(sc, minlength=ds.num_scenes)
    exp = len(sc) * ds.scene_probas
    x2 = float(((obs - exp) ** 2 / exp).sum())
    print("scene X^2 %.2f (bound %.2f), counts %s" % (x2, stats.chi2.ppf(0.999, ds.num_scenes - 1), obs.tolist()))
    assert x2 < stats.chi2.ppf(0.999, ds.num_scenes - 1)
    d = stats.kstest(an / (2 * np.pi), "uniform").statistic
    print("angle sqrt(n) D = %.3f (bound 1.949)" % (np.sqrt(len(an)) * d))
    assert np.sqrt(len(an)) * d < 1.949

    small = R.synthetic_scene(31, 2000, 3.0, 3.0) + ("small",)
    one = pn2.dataset.SemanticDataset(256, "train", True, 10, 10, "", device=cuda, seed=23, scenes=[small])
    hits = np.zeros(2000, np.int64)
    for _ in range(64):
        one.sample_batch_in_all_files(64, augment=False)
        assert (one.last_cnt == 2000).all()
        hits += np.bincount(one.last_sel.cpu().numpy().reshape(-1), minlength=2000)
    assert hits.sum() == 4096 * 256
    e = 4096 * 256 / 2000
    x2 = float(((hits - e) ** 2 / e).sum())
    print("member X^2 %.1f (bound %.1f)" % (x2, stats.chi2.ppf(0.999, 1999)))
    assert x2 < stats.chi2.ppf(0.999, 1999)


def test_dataset_feeds_the_trainer(pn2, cuda):
    """six training steps fed by the dataset through the prefetch path (steps 4-6 are captured replays), then eval_step on
    validation batches (all weights 0 -> loss 0)"""
    import torch
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16)
    B, N = 8, 2048
    scenes = R.synthetic_scenes()
    train = pn2.dataset.SemanticDataset(N, "train", True, 4, 4, "", device=cuda, seed=1, scenes=scenes)
    val = pn2.dataset.SemanticDataset(N, "validation", True, 4, 4, "", device=cuda, seed=2, scenes=scenes[1:])
    tr = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=3), warmup_eager=3)
    side = torch.cuda.Stream()
    cur = train.sample_batch_in_all_files(B, augment=True)
    losses = []
    for i in range(6):
        for t, (dt, shape) in zip(cur, ((torch.float32, (B, N, 6)), (torch.int32, (B, N)), (torch.float32, (B, N)))):
            assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()  # no conversion kernel in between
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            nxt = train.sample_batch_in_all_files(B, augment=True)
        torch.cuda.current_stream().wait_stream(side)
        for t in nxt:
            t.record_stream(torch.cuda.current_stream())
        losses.append(tr.train_step(*cur, next_pc=nxt[0], next_labels=nxt[1], next_smpw=nxt[2]))
        cur = nxt
    train.check_last()
    assert tr._graph is not None  # steps after the eager warm-up replay the captured step
    assert all(np.isfinite(losses)) and all(l > 0 for l in losses), losses
    for _ in range(2):
        pc, lab, w = val.sample_batch_in_all_files(B, augment=False)
        assert not w.any()
        assert tr.eval_step(pc, lab, w) == 0.0
    val.check_last()
