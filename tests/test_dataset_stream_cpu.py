"""CPU checks of tests/dataset_stream_ref.py (the numpy model of the device-random stream of pn2_dataset_sample) and of the
inputs test_dataset_stream_gpu.py compares on the device: each edge a GPU case aims at is asserted here from the model
alone, so that no GPU case passes because its edge never occurred.  A seed that fails a condition is replaced, the
condition stays."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataset_stream_cases as C  # noqa: E402
import dataset_stream_ref as M  # noqa: E402
import multiscene_ref as R  # noqa: E402

MASK = (1 << 64) - 1


# ---- the model's arithmetic --------------------------------------------------------------------------------------------
def _fmix_int(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & MASK
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & MASK
    return x ^ (x >> 33)


def _draw_int(seed, ctr, s, i):
    """the stream in Python integers reduced modulo 2^64 by hand"""
    h = _fmix_int((seed + 0x9E3779B97F4A7C15) & MASK)
    h = _fmix_int(h ^ ((ctr * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & MASK))
    h = _fmix_int(h ^ ((s * 0xAEF17502108EF2D9 + 0x632BE59BD9B4E019) & MASK))
    return _fmix_int(h ^ _fmix_int((i + 0x8CB92BA72F3D8DD7) & MASK))


def test_uint64_arrays_wrap_like_integers_modulo_2_64():
    """numpy must neither promote uint64 to float64 nor saturate: the model against Python integers"""
    rs = np.random.RandomState(0)
    for seed in (0, 1, 303, MASK, 0x9E3779B97F4A7C15):
        for ctr in (0, 1, 2, 2 ** 40, 2 ** 63 - 1):
            for s in (0, 1, 63, 65534):
                idx = [0, 1, 65999, 2 ** 31 - 1, M.TAG_SCENE, M.TAG_CENTER, M.TAG_ANGLE] + rs.randint(0, 2 ** 31, 4).tolist()
                h = M.sample_stream(seed, ctr, s)
                got = M.draw64(h, np.array(idx, dtype=np.uint64))
                assert got.dtype == np.uint64 and got.tolist() == [_draw_int(seed, ctr, s, i) for i in idx]
    assert M.fmix64(0).tolist() == [0] and M.fmix64(1).tolist() == [_fmix_int(1)]


def test_streams_differ_by_seed_counter_and_sample():
    hs = {int(M.sample_stream(seed, ctr, s)[0]) for seed in (0, 1) for ctr in range(4) for s in range(64)}
    assert len(hs) == 2 * 4 * 64


def test_unit53_lies_in_the_half_open_unit_interval():
    k = np.array([0, 1, 2047, 2048, 2 ** 63, MASK - 2048, MASK - 2047, MASK], dtype=np.uint64)
    u = M.unit53(k)
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
    assert u[0] == 0 and u[2] == 0 and u[3] == 2.0 ** -53 and u[-1] == 1 - 2.0 ** -53
    u = M.unit53(M.draw64(M.sample_stream(5, 0, 0), np.arange(100000)))
    assert (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 0.01


def test_center_rule_covers_exactly_the_scene():
    for n in (1, 2, 299, 300, 1024, 66000, 2 ** 31 - 1):
        assert M.pick_center(0, n) == 0 and M.pick_center(MASK, n) == n - 1
        # the smallest draw that gives index j is ceil(j 2^64 / n): the last index is reached, n never is
        first_last = -((-(n - 1) << 64) // n)
        assert M.pick_center(first_last, n) == n - 1 and (n == 1 or M.pick_center(first_last - 1, n) == n - 2)
    draws = M.draw64(M.sample_stream(1, 0, 0), np.arange(4000))
    got = {M.pick_center(k, 7) for k in draws}
    assert got == set(range(7))


def test_scene_rule_is_searchsorted_right():
    cdf = np.array([0.25, 0.25, 0.5, 1.0])  # an empty second scene: never chosen
    for u, k in ((0.0, 0), (0.2499, 0), (0.25, 2), (0.4, 2), (0.5, 3), (0.75, 3), (1 - 2.0 ** -53, 3)):
        assert M.pick_scene(cdf, u) == k == min(int(np.searchsorted(cdf, u, side="right")), 3)
    assert M.pick_scene(np.array([0.5, 1 - 2.0 ** -52]), 1 - 2.0 ** -53) == 1  # past a short cdf: the last scene
    rs = np.random.RandomState(3)
    for _ in range(50):
        p = rs.randint(1, 10 ** 6, rs.randint(1, 9)).astype(np.float64)
        cdf = (p / p.sum()).cumsum()
        cdf /= cdf[-1]
        for u in np.concatenate([rs.random_sample(20), cdf[:-1], np.nextafter(cdf[:-1], 0)]):
            want = int(np.searchsorted(cdf, u, side="right"))
            first_above = int(np.nonzero(cdf > u)[0][0])
            assert M.pick_scene(cdf, u) == want == first_above


def test_subset_rule():
    h = M.sample_stream(7, 3, 2)
    members = np.arange(5, 4000, 3)
    for n in (1, 2, 300, len(members) - 1):
        got = M.pick_subset(h, members, n)
        assert len(got) == n == len(set(got.tolist())) and (np.diff(got) > 0).all() and np.isin(got, members).all()
        keys = M.draw64(h, members)
        kth = np.sort(keys)[n - 1]
        assert np.array_equal(got, members[keys <= kth])  # the n smallest keys (no ties here)
        assert np.array_equal(got, M.pick_subset(h, members, n))
    # keys hang on the scene-local index, not on the position in the column
    assert not np.array_equal(M.pick_subset(h, members, 300), M.pick_subset(h, members + 1, 300) - 1)
    # a column of at most n members: the index list repeated
    assert M.pick_subset(h, members[:3], 7).tolist() == [5, 8, 11, 5, 8, 11, 5]
    assert np.array_equal(M.pick_subset(h, members[:300], 300), members[:300])
    # ties go to the lower index: forced here with equal keys, since hashed keys never tie in a test-sized column
    order = np.lexsort((np.array([4, 2, 9]), np.array([1, 1, 1], dtype=np.uint64)))
    assert order.tolist() == [1, 0, 2]


def test_rotation_is_the_reference_matrix_product():
    p = np.random.RandomState(1).uniform(-5, 5, (64, 3))
    for ang in (0.0, 0.3, 3.0, 6.2):
        assert np.allclose(M.rotate_z(p, ang), p @ R.rotation(ang), rtol=0, atol=1e-14)
    assert np.array_equal(M.rotate_z(p, 0.0), p)


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------
def _whole_scene_extent(pts, hx, hy):
    """-> slab length per centre of an x-sorted scene, by the kernel's two binary searches.  Every slab point is a member:
    y is asserted by the extreme points, z always holds (the column reaches scene_z_size above and below its centre)."""
    xs = pts[:, 0]
    slab = np.searchsorted(xs, xs + hx) - np.searchsorted(xs, xs - hx)
    assert pts[:, 1].max() - pts[:, 1].min() <= hy
    return slab


@pytest.mark.parametrize("n", C.N_VALUES)
def test_whole_scene_store_has_the_stated_columns(pn2, n):
    counts = C.whole_counts(n)
    assert {1, n, n + 1, 2 * n, 1024, 1025, 2048, 2049, 66000} <= set(counts) and (n == 1 or n - 1 in counts)
    ds = C.make(pn2, n, C.whole_scenes(n), C.SEED_WHOLE)
    assert ds.scene_counts.tolist() == counts
    assert ds.max_chunks == 65 == C.WORKGROUPS + 1  # the stride over chunks wraps for the last chunk of the largest scene
    for k, c in enumerate(counts):
        assert (_whole_scene_extent(ds.scene_points[k], C.BOX / 2, C.BOX / 2) == c).all()  # for every centre
        p = ds.scene_points[k]
        for ctr in (0, c // 2, c - 1):  # and by the reference's own column rule at three of them
            assert R.column(p, p[ctr], C.BOX / 2, C.BOX / 2).sum() == c
    for ctr, k, b in C.whole_plan(n):
        m = M.batch(ds, ctr, b, scene=k)
        assert (m["cnt"] == counts[k]).all() and (0 <= m["center"]).all() and (m["center"] < counts[k]).all()
        assert counts[k] < 64 or len(set(m["center"].tolist())) > 1
        for s in range(b):
            keys = M.draw64(M.sample_stream(ds.seed, ctr, s), m["members"][s])
            assert len(np.unique(keys)) == len(keys)
            assert len(set(m["sel"][s].tolist())) == min(n, counts[k])


def test_diagonal_scene_has_empty_and_full_chunks(pn2):
    ds = C.make(pn2, C.N_MAIN, [C.diagonal_scene()], C.SEED_DIAGONAL)
    n = int(ds.scene_counts[0])
    xs = ds.scene_points[0][:, 0]
    assert n == 20000 and xs.max() - xs.min() < C.BOX / 2
    nch = (n + C.CHUNK - 1) // C.CHUNK
    for ctr, b in enumerate(C.DIAGONAL_BATCHES):
        m = M.batch(ds, ctr, b, scene=0)
        for s in range(b):
            members = m["members"][s]
            per_chunk = np.bincount(members // C.CHUNK, minlength=nch)  # the slab is the whole scene: chunk = index // 1024
            assert m["cnt"][s] > C.N_MAIN and (per_chunk == 0).any() and (per_chunk > 0).any()
            # members are contiguous in x up to the noise: chunks without members lie on the outside
            live = np.nonzero(per_chunk)[0]
            assert (per_chunk[live[0]:live[-1] + 1] > 0).all()
            keys = M.draw64(M.sample_stream(ds.seed, ctr, s), members)
            assert len(np.unique(keys)) == len(keys)
    both_ends = [M.batch(ds, ctr, b, scene=0)["members"] for ctr, b in enumerate(C.DIAGONAL_BATCHES)]
    firsts = [mm[0] // C.CHUNK for mmm in both_ends for mm in mmm]
    assert min(firsts) == 0 and max(firsts) > 0  # columns that start in the first chunk and columns that skip it


def test_mixed_store_batches_meet_their_conditions(pn2):
    """Every scene is drawn, both column kinds occur, labels above 8 are selected, and no two members of a compared column
    share a key.  The last point is why the tie-break by index is not covered on the device: with 64-bit hashed keys a
    tie inside a column of c members has probability about c^2 / 2^65, so no seed of reasonable search length produces
    one; the rule itself is pinned on the model with forced keys (test_subset_rule)."""
    ds = C.make(pn2, C.N_MAIN, C.mixed_scenes(), C.SEED_MIXED)
    assert ds.num_scenes == 5 and len(set(ds.scene_counts.tolist())) == 5
    wide = ds.scene_labels[4]
    assert wide.min() == 0 and wide.max() == 255 and set(range(9, 256)) <= set(wide.tolist())
    scenes, cnts, labels, sels = [], [], [], []
    for ctr, b in enumerate(C.MIXED_BATCHES):
        m = M.batch(ds, ctr, b, augment=True)
        scenes += m["scene"].tolist()
        cnts += m["cnt"].tolist()
        labels.append(m["labels"])
        assert ((m["labels"] > 8) == (m["weights"] == 0)).all()  # train weights are positive below 9
        assert (0 <= m["angle"]).all() and (m["angle"] < 2 * np.pi).all() and len(set(m["angle"].tolist())) == b
        for s in range(b):
            keys = M.draw64(M.sample_stream(ds.seed, ctr, s), m["members"][s])
            assert len(np.unique(keys)) == len(keys)
        sels.append(m["sel"])
    assert not any(np.array_equal(sels[i], sels[j]) for i in range(3) for j in range(i))  # three different streams
    assert set(scenes) == set(range(5))
    cnts = np.array(cnts)
    assert (cnts <= C.N_MAIN).sum() >= 3 and (cnts > C.N_MAIN).sum() >= 3
    labels = np.concatenate(labels).ravel()
    assert (labels == 9).any() and (labels == 255).any() and (labels < 9).any()
    # the same batch again: the model holds no state
    a, b = M.batch(ds, 1, C.MIXED_BATCHES[1], augment=True), M.batch(ds, 1, C.MIXED_BATCHES[1], augment=True)
    for k in a:
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k


def test_rejection_inputs(pn2):
    ds = C.make(pn2, C.N_MAIN, C.mixed_scenes(), C.SEED_MIXED)
    draws, cnt = C.replay_draws(ds)
    order = np.sort(cnt)
    assert order[-1] > order[-2] > C.N_MAIN  # capacity max - 1 rejects one sample and keeps another wide column
    assert (cnt <= C.N_MAIN).any()
    assert all(draws["masks"][s, :c].sum() == C.N_MAIN and not draws["masks"][s, c:].any()
               for s, c in enumerate(cnt) if c > C.N_MAIN)
    # status 5: a slab of more than one chunk and a slab of one chunk in the same batch
    two = C.make(pn2, C.N_MAIN, C.chunk_scenes(), C.SEED_CHUNKS)
    assert two.scene_counts.tolist() == [3000, 700] and two.max_chunks == 3
    for k in range(2):
        assert (_whole_scene_extent(two.scene_points[k], C.BOX / 2, C.BOX / 2) == two.scene_counts[k]).all()
    m = M.batch(two, 0, C.CHUNKS_BATCH)
    assert set(m["scene"].tolist()) == {0, 1}
