"""CPU tests of the augmentation (util/provider.py, pn2_augment): the numpy model tests/provider_ref.py against the frozen
outputs of the reference's util/provider.py, the statistics of the model's device stream, and the argument validation of
the C entry points (refused before any launch, so no GPU is needed)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataset_stream_ref as S  # noqa: E402
import provider_cases as C  # noqa: E402
import provider_ref as M  # noqa: E402

GOLD = C.golden()
CASES = C.golden_cases(GOLD)


def test_golden_file_is_small_and_holds_the_edges_the_tests_name():
    assert os.path.getsize(C.GOLDEN) < 256 * 1024
    assert GOLD["in3"].shape == (2, 257, 3) and GOLD["in6"].shape == (2, 257, 6)
    assert GOLD["in3"].dtype == np.float32 and np.abs(GOLD["in6"]).max() < 5
    dropped = GOLD["dropout_u"] <= GOLD["dropout_ratio"][:, None]
    assert dropped[:, 0].any() and not dropped[:, 0].all()          # row 0 dropped in one cloud
    none = GOLD["dropout_none_u"] <= GOLD["dropout_none_ratio"][:, None]
    assert (~none.any(1)).any() and none.any()                      # a ratio below every u: nothing drops
    assert np.array_equal(np.sort(GOLD["shuffle_perm"]), np.arange(257))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_replays_the_reference_bit_for_bit(case):
    name, key, cfg, draws = case[:4]
    want = GOLD[name + "_out"]
    if name == "jitter":
        assert want.dtype == np.float64  # the reference returns float64: its float32 cast is the contract
    got = M.apply(GOLD[key], cfg, draws)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))
    assert not np.array_equal(got, GOLD[key])  # the case does something


def test_shuffle_is_the_gather_by_the_index_and_companions_follow():
    x, idx = GOLD["in6"], GOLD["shuffle_perm"]
    lab = np.arange(2 * 257, dtype=np.int32).reshape(2, 257)
    w = lab.astype(np.float32) / 3
    out, lo, wo = M.apply(x, {"shuffle": True}, {"perm": idx}, lab, w)
    assert np.array_equal(out, x[:, idx, :]) and np.array_equal(lo, lab[:, idx]) and np.array_equal(wo, w[:, idx])


def test_values_stay_float64_between_stages():
    """the fused rule is not a chain of float32 roundings: on these inputs the two differ, and the model is the former"""
    x, _, _ = C.edge_input(3, 1000, 3)
    cfg = dict(C.STAGES["fused"])
    d = C.edge_draws(3, 1000, 3, cfg)
    fused = M.apply(x, cfg, d)
    chained = x
    for k in ("shuffle", "rotate", "scale", "shift", "jitter", "dropout"):
        one = {k: cfg[k]}
        if k == "rotate":
            one["perturb"] = cfg["perturb"]
        chained = M.apply(chained, one, d)
    diff = (fused != chained).mean()
    assert 0.01 < diff < 0.9 and np.abs(fused - chained).max() < 5e-6  # a few float32 ulps at |x| < 16


def test_dropout_row0_rule():
    x, _, _ = C.edge_input(3, 65, 6)
    cfg = {"shift": 0.1, "jitter": (0.01, 0.05), "dropout": 0.875}
    d = C.edge_draws(3, 65, 6, cfg)
    out = M.apply(x, cfg, d)
    before = M.apply(x, {k: v for k, v in cfg.items() if k != "dropout"}, d)
    assert np.array_equal(out[:, 0], before[:, 0])                       # row 0 keeps its value, dropped or not
    assert np.array_equal(out[1, 1:5], before[1, 1:5]) and np.array_equal(out[1, 5], before[1, 0])  # ratio 0, u == 0
    assert (out[2] == before[2, 0]).all()                                # a ratio above every u
    dropped = d["u"][0] <= 0.5
    assert np.array_equal(out[0, ~dropped], before[0, ~dropped]) and (out[0, dropped] == before[0, 0]).all()


# ---- the device stream of the model --------------------------------------------------------------------------------------
def test_stream_statistics():
    n = 100000
    h = S.sample_stream(7, 3, 0)
    z = M.normal(h, np.uint64(M.TAG_JITTER) + np.uint64(2) * np.arange(n, dtype=np.uint64))
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1) < 5 * np.sqrt(2.0 / n)
    u = M.unit(h, np.arange(n, dtype=np.uint64) + np.uint64(M.TAG_DROP))
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 5 / np.sqrt(12 * n)
    v = M.uniform(0.8, 1.25, u)
    assert v.min() >= 0.8 and v.max() <= 1.25
    t = M.uniform(-0.1, 0.1, u)
    assert t.min() >= -0.1 and t.max() <= 0.1
    p = M.permutation(7, 3, n)
    assert np.array_equal(np.sort(p), np.arange(n)) and not np.array_equal(p, np.arange(n))
    assert not np.array_equal(p, M.permutation(7, 4, n))  # the next call's permutation is another one


def test_tags_do_not_share_draws():
    h = S.sample_stream(0, 0, 0)
    tags = [S.TAG_SCENE, S.TAG_CENTER, S.TAG_ANGLE, M.TAG_ANGLE, M.TAG_SCALE, M.TAG_RATIO, M.TAG_JITTER, M.TAG_DROP, M.TAG_PERM]
    tags += [M.TAG_PERTURB + k for k in range(6)] + [M.TAG_SHIFT + k for k in range(3)]
    assert len(set(tags)) == len(tags)
    draws = [int(S.draw64(h, t)[0]) for t in tags]
    assert len(set(draws)) == len(draws)
    # the spaces do not overlap for any batch the entry point accepts (n * c < 2^40), and lie above the dataset's
    assert M.TAG_ANGLE > S.TAG_ANGLE and M.TAG_RATIO < M.TAG_JITTER
    assert M.TAG_JITTER + 2 * 2 ** 40 <= M.TAG_DROP and M.TAG_DROP + 2 ** 31 <= M.TAG_PERM
    # a dataset and an augmenter sharing seed, counter and cloud: different values for their first per-point draws
    i = np.arange(1000, dtype=np.uint64)
    assert not np.intersect1d(S.draw64(h, i), S.draw64(h, i + np.uint64(M.TAG_DROP))).size


def test_device_call_is_a_function_of_the_counter():
    x, lab, w = C.edge_input(3, 65, 6)
    cfg = dict(C.STAGES["fused"])
    a, da = M.device_call(x, cfg, 11, 0, lab, w)
    b, db = M.device_call(x, cfg, 11, 0, lab, w)
    c, dc = M.device_call(x, cfg, 11, 1, lab, w)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(da["perm"], dc["perm"])
    assert np.array_equal(a[1], lab[:, da["perm"]]) and np.array_equal(a[2], w[:, da["perm"]])
    for r in da["matrix"]:  # R_axis . R_perturb is a rotation
        assert np.allclose(r @ r.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(r) - 1) < 1e-14
    assert ((0.8 <= da["scale"]) & (da["scale"] <= 1.25)).all() and (np.abs(da["shift"]) <= 0.1).all()
    assert ((0 <= da["ratio"]) & (da["ratio"] <= 0.875)).all()


# ---- the C ABI: refused before any launch ------------------------------------------------------------------------------------
def _call(pn2, **kw):
    """pn2_augment with placeholder pointers (never dereferenced: every call here is refused), changed by kw"""
    K = pn2._lib.ABI.constants
    fake = ctypes.c_void_p(4096)
    a = dict(b=2, n=64, c=6, flags=0, rotate_axis=2, perturb_sigma=0.06, perturb_clip=0.18, scale_lo=0.8, scale_hi=1.25,
             shift_range=0.1, jitter_sigma=0.01, jitter_clip=0.05, dropout_max=0.875, seed=0, counter=fake, draw_perm=None,
             draw_matrix=None, draw_scale=None, draw_shift=None, draw_noise=None, draw_ratio=None, draw_u=None, **{"in": fake},
             in_labels=None, in_weights=None, workspace=None, workspace_bytes=0, out_params=None, out_perm=None,
             out=ctypes.c_void_p(8192), out_labels=None, out_weights=None, stream=None)
    for k, v in kw.items():
        assert k in a, k
        a[k] = K[v] if isinstance(v, str) else v
    names = pn2._lib.ABI.functions["pn2_augment"].argnames
    assert set(names) == set(a)
    return pn2._lib.lib.pn2_augment(*[a[k] for k in names])


def test_augment_argument_validation_needs_no_gpu(pn2):
    K = pn2._lib.ABI.constants
    EINVAL, ENULL = K["PN2_EINVAL"], K["PN2_ENULL"]
    fake = ctypes.c_void_p(4096)
    every = sum(K["PN2_AUG_" + k] for k in ("SHUFFLE", "ROTATE", "PERTURB", "SCALE", "SHIFT", "JITTER", "DROPOUT"))
    # dimensions first, whatever the pointers are
    for bad in (dict(b=0), dict(b=-1), dict(n=0), dict(c=2), dict(b=65536), dict(flags=1 << 20)):
        assert _call(pn2, **bad) == EINVAL, bad
        assert _call(pn2, **dict(bad, **{"in": None})) == EINVAL, bad
    assert _call(pn2, c=5, flags=K["PN2_AUG_ROTATE"] | K["PN2_AUG_ROTATE_NORMALS"]) == EINVAL  # normals need c >= 6
    assert _call(pn2, c=6, flags=K["PN2_AUG_ROTATE"] | K["PN2_AUG_ROTATE_NORMALS"]) == ENULL   # ... reaches the workspace check
    assert _call(pn2, flags="PN2_AUG_ROTATE", rotate_axis=3) == EINVAL
    assert _call(pn2, flags="PN2_AUG_JITTER", jitter_clip=0.0) == EINVAL
    assert _call(pn2, flags="PN2_AUG_SCALE", scale_lo=2.0, scale_hi=1.0) == EINVAL
    assert _call(pn2, flags="PN2_AUG_DROPOUT", dropout_max=1.5) == EINVAL
    # in == out with the shuffle
    assert _call(pn2, flags="PN2_AUG_SHUFFLE", out=fake, out_perm=fake, workspace=fake) == EINVAL
    assert _call(pn2, flags="PN2_AUG_SHIFT", out=fake) == ENULL  # in place without it: goes on to the workspace (NULL here)
    # labels / weights come in pairs
    assert _call(pn2, in_labels=fake) == EINVAL and _call(pn2, out_weights=fake) == EINVAL
    # required pointers
    assert _call(pn2, **{"in": None}) == ENULL and _call(pn2, out=None) == ENULL and _call(pn2, workspace=None) == ENULL
    ws = ctypes.c_void_p(1 << 20)
    assert _call(pn2, flags=every, counter=None, workspace=ws, out_perm=fake) == ENULL        # device mode needs the counter
    assert _call(pn2, flags="PN2_AUG_SHUFFLE", workspace=ws, out_perm=None) == ENULL
    replay = K["PN2_AUG_REPLAY"]
    need = {"PN2_AUG_SHUFFLE": ["draw_perm"], "PN2_AUG_ROTATE": ["draw_matrix"], "PN2_AUG_PERTURB": ["draw_matrix"],
            "PN2_AUG_SCALE": ["draw_scale"], "PN2_AUG_SHIFT": ["draw_shift"], "PN2_AUG_JITTER": ["draw_noise"],
            "PN2_AUG_DROPOUT": ["draw_ratio", "draw_u"]}
    draws = dict.fromkeys((k for v in need.values() for k in v), fake)
    for stage, keys in need.items():
        for k in keys:  # a replay pointer missing for an enabled stage; the counter is not needed
            assert _call(pn2, flags=K[stage] | replay, counter=None, workspace=ws, out_perm=fake, workspace_bytes=0,
                         **dict(draws, **{k: None})) == ENULL, (stage, k)
        # all of them given: the call reaches the workspace size check
        assert _call(pn2, flags=K[stage] | replay, counter=None, workspace=ws, out_perm=fake, **draws) == EINVAL, stage
    # a replay input of a stage that is off is not required
    assert _call(pn2, flags=K["PN2_AUG_SHIFT"] | replay, counter=None, workspace=ws, draw_shift=fake) == EINVAL
    # the workspace: too small, misaligned
    nbytes = ctypes.c_ulonglong(0)
    L = pn2._lib.lib
    assert L.pn2_augment_workspace_bytes(0, ctypes.byref(nbytes)) == EINVAL
    assert L.pn2_augment_workspace_bytes(2, None) == ENULL
    assert L.pn2_augment_workspace_bytes(2, ctypes.byref(nbytes)) == 0 and nbytes.value >= 2 * 16 * 8 + 8
    assert _call(pn2, flags="PN2_AUG_SHIFT", workspace=ws, workspace_bytes=nbytes.value - 1) == EINVAL
    assert _call(pn2, flags="PN2_AUG_SHIFT", workspace=ctypes.c_void_p((1 << 20) + 64), workspace_bytes=nbytes.value) == EINVAL
    # in place with dropout keeps row 0 of every cloud in the workspace: at most PN2_AUG_INPLACE_MAX_C channels
    wide = K["PN2_AUG_INPLACE_MAX_C"] + 1
    assert _call(pn2, c=wide, flags="PN2_AUG_DROPOUT", out=fake, workspace=ws, workspace_bytes=nbytes.value) == K["PN2_EUNSUP"]


def test_provider_module_has_the_reference_names(pn2):
    P = pn2.util.provider
    for name in ["shuffle_data", "shuffle_points", "rotate_point_cloud", "rotate_feature_point_cloud",
                 "rotate_point_cloud_with_normal", "rotate_perturbation_point_cloud_with_normal", "rotate_point_cloud_by_angle",
                 "rotate_point_cloud_by_angle_with_normal", "rotate_perturbation_point_cloud", "jitter_point_cloud",
                 "shift_point_cloud", "random_scale_point_cloud", "random_point_dropout", "Augmenter"]:
        assert callable(getattr(P, name)), name
    assert not hasattr(P, "load_h5") and not hasattr(P, "getDataFiles")
    import inspect
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.name != "draws"]  # noqa: E731
    E = inspect.Parameter.empty
    assert sig(P.rotate_point_cloud) == [("batch_data", E), ("rotation_axis", "z")]
    assert sig(P.rotate_feature_point_cloud) == [("batch_data", E), ("feature_size", 3), ("rotation_axis", "z")]
    assert sig(P.rotate_perturbation_point_cloud) == [("batch_data", E), ("angle_sigma", 0.06), ("angle_clip", 0.18)]
    assert sig(P.jitter_point_cloud) == [("batch_data", E), ("sigma", 0.01), ("clip", 0.05)]
    assert sig(P.shift_point_cloud) == [("batch_data", E), ("shift_range", 0.1)]
    assert sig(P.random_scale_point_cloud) == [("batch_data", E), ("scale_low", 0.8), ("scale_high", 1.25)]
    assert sig(P.random_point_dropout) == [("batch_pc", E), ("max_dropout_ratio", 0.875)]
    # the replay matrices are numpy's: the host helpers give what the reference's expressions give
    a = np.float64(0.3)
    assert np.array_equal(P.axis_matrix("y", a), np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]))
    with pytest.raises(ValueError):
        P.axis_matrix("w", a)
    with pytest.raises(ValueError, match="MI355X only"):
        import torch
        P.shift_point_cloud(torch.zeros(1, 4, 3))
