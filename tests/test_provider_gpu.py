"""GPU tests of the augmentation (util/provider.py, csrc/pn2_augment.hip) against the reference's frozen outputs
(tests/golden/provider.npz) and against tests/provider_ref.py, the numpy model of the rule in include/pn2_abi.h.

Edge shapes: B in {1, 3}, N in {1, 63, 64, 65, 257, 1000} (the lane, wave and workgroup edges), C in {3, 6, 7} (12-byte rows,
the 16 + 8 byte rows, an odd width with channels past the sixth).  The raw calls write every output -- batch, labels,
weights, parameters, permutation -- into buffers poisoned on both sides, on bases that are 256-byte, 8-byte and only 4-byte
aligned, and the poison is checked afterwards.

Replay is bit-exact.  Device mode: scale, shift, ratio, permutation and the dropout mask are exact; a matrix entry may sit
4 float64 ulp from the model's (the device's cos / sin / log against numpy's); an output value 1 float32 ulp, and at most
0.1 % of the values may differ at all: a float64 error of a few 2^-53 moves a float32 rounding with probability about 2^-27
per value, so the model alone expects about 10^-3 differing values at these sizes (the tests print the count)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataset_stream_cases as DC  # noqa: E402
import dataset_stream_ref as DS  # noqa: E402
import provider_cases as C  # noqa: E402
import provider_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0x7FC5A5A5  # a quiet NaN with a payload: an int32 pattern no kernel here writes


@pytest.fixture(scope="module")
def gold():
    return C.golden()


def _ulps(a, b):
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _ulps64(a, b):
    ia, ib = a.astype(np.float64).view(np.int64), b.astype(np.float64).view(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFFFFFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFFFFFFFFFF), ib)
    return np.abs(ia - ib)


class Guarded:
    """a tensor of `shape` inside a poisoned allocation; `skew` 4-byte words shift its base off the 256-byte boundary"""

    def __init__(self, torch, dev, shape, dtype, skew=0, fill=None):
        words = {torch.float32: 1, torch.int32: 1, torch.float64: 2}[dtype]
        n = int(np.prod(shape)) * words
        self.lo, self.hi = 64 + skew, 64 + skew + n
        self.raw = torch.full((self.hi + 64,), POISON, dtype=torch.int32, device=dev)
        self.t = self.raw[self.lo:self.hi].view(dtype).view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def check(self, what):
        assert bool((self.raw[:self.lo] == POISON).all()) and bool((self.raw[self.hi:] == POISON).all()), what + ": guard overwritten"


def _flags(P, cfg):
    f = 0
    for key, bit in (("shuffle", P.SHUFFLE), ("rotate", P.ROTATE), ("perturb", P.PERTURB), ("normals", P.ROTATE_NORMALS),
                     ("scale", P.SCALE), ("shift", P.SHIFT), ("jitter", P.JITTER), ("jitter_all", P.JITTER_ALL),
                     ("dropout", P.DROPOUT)):
        if cfg.get(key):
            f |= bit
    return f


def _raw(pn2, dev, x, lab, w, cfg, draws=None, seed=0, counter=None, skew=0, in_place=False, check=True):
    """one raw pn2_augment call with every output guarded -> (out, labels, weights, params, perm) as numpy, and the return code
    instead when check is False"""
    import torch
    L, P = pn2._lib, pn2.util.provider
    b, n, c = x.shape
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    flags = _flags(P, cfg)
    shuffle = bool(flags & P.SHUFFLE)
    gx = Guarded(torch, dev, (b, n, c), torch.float32, skew, fill=t(x, np.float32))
    go = gx if in_place else Guarded(torch, dev, (b, n, c), torch.float32, skew)
    gl = Guarded(torch, dev, (b, n), torch.int32, skew)
    gw = Guarded(torch, dev, (b, n), torch.float32, skew)
    gp = Guarded(torch, dev, (b, 16), torch.float64, 2 * (skew // 2))
    gperm = Guarded(torch, dev, (n,), torch.int32, skew)
    d = dict.fromkeys(("perm", "matrix", "scale", "shift", "noise", "ratio", "u"))
    if draws is not None:
        flags |= P.REPLAY
        d = {k: t(draws[k], np.int32 if k == "perm" else np.float64) for k in d}
    nbytes = L.u64_array([0])
    L.launch("pn2_augment_workspace_bytes", dev, b, nbytes, stream=False)
    ws = torch.zeros(nbytes[0] + 256, dtype=torch.uint8, device=dev)
    base = (-ws.data_ptr()) % 256
    p = L.ptr
    tl, tw = t(lab, np.int32), t(w, np.float32)
    pert, sc, jit = cfg.get("perturb", (0.0, 1.0)), cfg.get("scale", (1.0, 1.0)), cfg.get("jitter", (0.0, 1.0))
    args = (b, n, c, flags, {"x": 0, "y": 1, "z": 2}[cfg.get("rotate", "z")], pert[0], pert[1], sc[0], sc[1],
            float(cfg.get("shift", 0.0)), jit[0], jit[1], float(cfg.get("dropout", 0.0)), seed, p(counter), p(d["perm"]),
            p(d["matrix"]), p(d["scale"]), p(d["shift"]), p(d["noise"]), p(d["ratio"]), p(d["u"]), p(gx.t), p(tl), p(tw),
            p(ws[base:]), ws.numel() - base, p(gp.t), p(gperm.t) if shuffle else None, p(go.t), p(gl.t), p(gw.t))
    if not check:
        with torch.cuda.device(dev):
            return L.lib.pn2_augment(*args, L.stream_ptr())
    L.launch("pn2_augment", dev, *args)
    torch.cuda.synchronize()
    what = "b %d n %d c %d %s skew %d" % (b, n, c, sorted(cfg), skew)
    for g in (gx, go, gl, gw, gp, gperm):
        g.check(what)
    if not in_place:
        assert np.array_equal(gx.t.cpu().numpy().view(np.int32), x.view(np.int32)), what + ": the input was written"
    if not shuffle:
        assert bool((gperm.t == POISON).all()), what + ": a permutation was written without the shuffle"
    return go.t.cpu().numpy(), gl.t.cpu().numpy(), gw.t.cpu().numpy(), gp.t.cpu().numpy(), gperm.t.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- 1 replay of the reference, one stage at a time ------------------------------------------------------------------------
def test_functions_replay_the_reference(pn2, cuda, gold):
    import torch
    P = pn2.util.provider
    in_place = {"rotate_point_cloud_with_normal", "shift_point_cloud", "random_scale_point_cloud", "random_point_dropout"}
    for name, key, cfg, _, fn, args, draws in C.golden_cases(gold):
        g = Guarded(torch, cuda, gold[key].shape, torch.float32, fill=torch.from_numpy(gold[key]).to(cuda))
        kw = {} if draws is None else {"draws": draws}
        out = getattr(P, fn)(g.t, *args, **kw)
        torch.cuda.synchronize()
        g.check(name)
        assert out.dtype == torch.float32 and out.is_cuda
        want = torch.from_numpy(gold[name + "_out"].astype(np.float32)).to(cuda)  # jitter: the cast of its float64 output
        assert torch.equal(out, want), name
        assert _same_bits(out.cpu().numpy(), want.cpu().numpy()), name  # (torch.equal takes -0.0 for 0.0)
        if fn in in_place:
            assert out.data_ptr() == g.t.data_ptr(), name
        else:
            assert torch.equal(g.t, torch.from_numpy(gold[key]).to(cuda)), name


def test_shuffle_is_the_gather_and_companions_follow(pn2, cuda, gold):
    import torch
    x, idx = torch.from_numpy(gold["in6"]).to(cuda), gold["shuffle_perm"]
    assert torch.equal(pn2.util.provider.shuffle_points(x, draws={"perm": idx}), x[:, torch.from_numpy(idx).to(cuda), :])
    lab = torch.arange(2 * 257, dtype=torch.int32, device=cuda).reshape(2, 257)
    w = lab.float() / 3
    aug = pn2.util.provider.Augmenter(device=cuda, shuffle=True)
    out, lo, wo = aug(x, lab, w, draws={"perm": idx})
    ti = torch.from_numpy(idx).to(cuda)
    assert torch.equal(out, x[:, ti, :]) and torch.equal(lo, lab[:, ti]) and torch.equal(wo, w[:, ti])
    assert torch.equal(aug.last_perm.long(), ti.long())
    with pytest.raises(ValueError):
        aug(x, out=x, draws={"perm": idx})
    with pytest.raises(ValueError):
        aug(x, draws={"perm": np.zeros(257, dtype=np.int64)})  # not a permutation


def test_by_angle_with_normal_against_the_model(pn2, cuda, gold):
    """the reference's function raises for every shape; the package's rotates xyz and normals about y"""
    import torch
    x = gold["in6"]
    out = pn2.util.provider.rotate_point_cloud_by_angle_with_normal(torch.from_numpy(x).to(cuda), 0.4)
    want = M.apply(x, {"rotate": "y", "normals": True}, {"matrix": np.stack([M.axis_matrix("y", 0.4)] * 2)})
    assert _same_bits(out.cpu().numpy(), want)


# ---- 2 replay on the edge shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CHANNELS)
@pytest.mark.parametrize("b", C.BATCHES)
def test_replay_on_the_edge_shapes(pn2, cuda, b, c):
    for n in C.POINTS:
        x, lab, w = C.edge_input(b, n, c)
        skew = (0, 2, 1)[(n + c) % 3]  # bases aligned to 256, 8 and 4 bytes
        for stage, cfg in C.STAGES.items():
            if cfg.get("normals") and c < 6:
                continue
            what = "b %d n %d c %d %s" % (b, n, c, stage)
            d = C.edge_draws(b, n, c, cfg)
            want, wl, ww = M.apply(x, cfg, d, lab, w)
            out, ol, ow, params, perm = _raw(pn2, cuda, x, lab, w, cfg, d, skew=skew)
            assert _same_bits(out, want), what
            assert np.array_equal(ol, wl) and _same_bits(ow, ww), what
            if cfg.get("shuffle"):
                assert np.array_equal(perm, d["perm"]), what
            if "scale" in cfg:
                assert np.array_equal(params[:, 9], d["scale"]), what
            if "dropout" in cfg:
                assert np.array_equal(params[:, 13], d["ratio"]), what
            if not cfg.get("shuffle"):  # in place
                got = _raw(pn2, cuda, x, lab, w, cfg, d, skew=skew, in_place=True)[0]
                assert _same_bits(got, want), what + " in place"


def test_in_place_with_the_shuffle_is_refused(pn2, cuda):
    x, lab, w = C.edge_input(3, 65, 6)
    cfg = C.STAGES["fused"]
    rc = _raw(pn2, cuda, x, lab, w, cfg, C.edge_draws(3, 65, 6, cfg), in_place=True, check=False)
    assert rc == pn2._lib.ABI.constants["PN2_EINVAL"]


# ---- 3 device mode against the model's stream ----------------------------------------------------------------------------------
CONFIGS = {
    "all": dict(rotate="z", perturb=(0.06, 0.18), scale=(0.8, 1.25), shift=0.1, jitter=(0.01, 0.05), dropout=0.875, shuffle=True),
    "normals": dict(rotate="y", rotate_normals=True, jitter=(0.02, 0.05), dropout=0.3),
    "axis_x": dict(rotate="x", scale=(0.5, 2.0)),
}


def _model_cfg(kw):
    cfg = {k: v for k, v in kw.items() if k not in ("rotate_normals", "jitter_all_channels")}
    if kw.get("rotate_normals"):
        cfg["normals"] = True
    if kw.get("jitter_all_channels"):
        cfg["jitter_all"] = True
    return cfg


def _check_device_call(aug, cfg, seed, counter, x, got, labels=None, weights=None, tally=None):
    """one device-mode call of `aug` (outputs `got`) against the model at `counter`"""
    res, d = M.device_call(x, cfg, seed, counter, labels, weights)
    want, wl, ww = res if labels is not None else (res, None, None)
    what = "counter %d %s" % (counter, sorted(cfg))
    assert np.array_equal(aug.last_scale.cpu().numpy(), d["scale"]), what
    assert np.array_equal(aug.last_shift.cpu().numpy(), d["shift"]), what
    assert np.array_equal(aug.last_ratio.cpu().numpy(), d["ratio"]), what
    if cfg.get("shuffle"):
        assert np.array_equal(aug.last_perm.cpu().numpy(), d["perm"]), what
    else:
        assert aug.last_perm is None
    mu = _ulps64(aug.last_matrix.cpu().numpy(), d["matrix"])
    print("%s: matrix entries at most %d float64 ulp from the model" % (what, mu.max()))
    assert mu.max() <= 4, what
    out = got[0].cpu().numpy() if isinstance(got, tuple) else got.cpu().numpy()
    if "dropout" in cfg:  # the mask: a dropped row is row 0 of its cloud, bit for bit (jittered rows are never equal by chance)
        mask = d["u"] <= d["ratio"][:, None]
        mask[:, 0] = True
        same = (out.view(np.int32) == out[:, :1, :].view(np.int32)).all(2)
        assert "jitter" in cfg and np.array_equal(same, mask), what
    u = _ulps(out, want)
    off = int((u > 0).sum())
    print("%s: %d of %d values differ from the model (limit %d), worst %d ulp" % (what, off, u.size, int(1e-3 * u.size), u.max()))
    assert u.max() <= 1 and off <= 1e-3 * u.size, what
    if labels is not None:
        assert np.array_equal(got[1].cpu().numpy(), wl) and np.array_equal(got[2].cpu().numpy(), ww), what
    if tally is not None:
        tally[0] += off
        tally[1] += u.size


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_device_mode_follows_the_model_stream(pn2, cuda, name):
    import torch
    kw = CONFIGS[name]
    cfg = _model_cfg(kw)
    tally = [0, 0]
    for b, n, c in ((3, 1000, 6), (1, 65, 7), (3, 257, 3)):
        if kw.get("rotate_normals") and c < 6:
            continue
        seed = 100 + n
        aug = pn2.util.provider.Augmenter(seed=seed, device=cuda, **kw)
        assert aug.seed == seed and int(aug.batch_counter.item()) == 0
        x, lab, w = C.edge_input(b, n, c, seed=1)
        tx, tl, tw = (torch.from_numpy(a).to(cuda) for a in (x, lab, w))
        for counter in range(2):
            g = Guarded(torch, cuda, x.shape, torch.float32, skew=counter)
            got = aug(tx, tl, tw, out=g.t)
            torch.cuda.synchronize()
            g.check("%s call %d" % (name, counter))
            assert got[0].data_ptr() == g.t.data_ptr()
            assert int(aug.batch_counter.item()) == counter + 1
            _check_device_call(aug, cfg, seed, counter, x, got, lab, w, tally)
            assert torch.equal(tx.cpu(), torch.from_numpy(x))
    print("%s: %d of %d values differ from the model in all" % (name, tally[0], tally[1]))


def test_device_permutation_at_every_edge_size(pn2, cuda):
    """the rank count at one point, one short of a wave, a wave, one past it, two workgroups' worth and sixteen"""
    import torch
    aug = pn2.util.provider.Augmenter(seed=5, device=cuda, shuffle=True)
    for counter, n in enumerate(C.POINTS):
        x = torch.arange(2 * n * 3, dtype=torch.float32, device=cuda).reshape(2, n, 3)
        out = aug(x)
        want = M.permutation(5, counter, n)
        assert np.array_equal(aug.last_perm.cpu().numpy(), want), n
        assert torch.equal(out, x[:, torch.from_numpy(want).to(cuda).long(), :]), n


def test_seeds_and_objects_are_independent_streams(pn2, cuda):
    import torch
    x = torch.from_numpy(C.edge_input(3, 257, 6)[0]).to(cuda)
    mk = lambda s: pn2.util.provider.Augmenter(seed=s, device=cuda, rotate="z", jitter=(0.01, 0.05), dropout=0.5)  # noqa: E731
    a, b, c = mk(1), mk(1), mk(2)
    ya, yb, yc = a(x), b(x), c(x)
    assert torch.equal(ya, yb) and not torch.equal(ya, yc)
    assert not torch.equal(a(x), ya)  # the next call draws again


# ---- 4 graph capture -----------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_into_fresh_draws(pn2, cuda):
    import torch
    kw = CONFIGS["all"]
    cfg = _model_cfg(kw)
    x, lab, w = C.edge_input(3, 1000, 6, seed=2)
    tx, tl, tw = (torch.from_numpy(a).to(cuda) for a in (x, lab, w))
    aug = pn2.util.provider.Augmenter(seed=77, device=cuda, **kw)
    aug(tx, tl, tw)  # eager once: the workspace and the counter exist before the capture
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            got = aug(tx, tl, tw)
    torch.cuda.current_stream().wait_stream(s)
    assert int(aug.batch_counter.item()) == 1  # the capture launched nothing
    outs = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(aug.batch_counter.item()) == 2 + k
        _check_device_call(aug, cfg, 77, 1 + k, x, got, lab, w)
        outs.append(got[0].clone())
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[2])


# ---- 5 the dataset with an Augmenter ---------------------------------------------------------------------------------------------
def test_dataset_accepts_an_augmenter(pn2, cuda):
    import torch
    mk = lambda: DC.make(pn2, DC.N_MAIN, DC.mixed_scenes(), DC.SEED_MIXED, device=cuda)  # noqa: E731
    before = mk()
    plain = [[t.clone() for t in before.sample_batch_in_all_files(3, augment=a)] for a in (True, False)]
    kw = dict(rotate="z", scale=(0.8, 1.25), shift=0.1, jitter=(0.01, 0.05), dropout=0.5, shuffle=True)
    cfg = _model_cfg(kw)
    for shuffle in (True, False):
        kw["shuffle"] = cfg["shuffle"] = shuffle
        aug = pn2.util.provider.Augmenter(seed=DC.SEED_MIXED, device=cuda, **kw)
        ds, base = mk(), mk()
        for counter in range(2):
            got = ds.sample_batch_in_all_files(3, augment=aug)
            ds.check_last()
            raw = [t.cpu().numpy() for t in base.sample_batch_in_all_files(3, augment=False)]
            m = DS.batch(base, counter, 3)
            assert np.array_equal(raw[0], m["data"]) and np.array_equal(ds.last_sel.cpu().numpy(), m["sel"])
            assert int(ds.batch_counter.item()) == counter + 1 and int(aug.batch_counter.item()) == counter + 1
            assert got[0].shape == (3, DC.N_MAIN, 6) and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
            _check_device_call(aug, cfg, DC.SEED_MIXED, counter, raw[0], got, raw[1], raw[2])
    # the sampler's own paths are what they were before any Augmenter existed in this test
    after = mk()
    for a, want in zip((True, False), plain):
        for t, u in zip(after.sample_batch_in_all_files(3, augment=a), want):
            assert torch.equal(t, u)
    m = DS.batch(after, 1, 3)
    assert np.array_equal(plain[1][0].cpu().numpy(), m["data"]) and np.array_equal(plain[1][1].cpu().numpy(), m["labels"])


# ---- 6 training fed through the prefetch path --------------------------------------------------------------------------------------
def test_augmented_batches_feed_the_trainer(pn2, cuda):
    import torch
    import multiscene_ref as R
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16)
    B, N = 8, 2048
    train = pn2.dataset.SemanticDataset(N, "train", True, 4, 4, "", device=cuda, seed=1, scenes=R.synthetic_scenes())
    aug = pn2.util.provider.Augmenter(seed=1, device=cuda, rotate="z", scale=(0.8, 1.25), shift=0.1, jitter=(0.01, 0.05),
                                      dropout=0.875, shuffle=True)
    tr = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=3), warmup_eager=2)
    side = torch.cuda.Stream()
    cur = train.sample_batch_in_all_files(B, augment=aug)
    losses = []
    for _ in range(3):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            nxt = train.sample_batch_in_all_files(B, augment=aug)
        torch.cuda.current_stream().wait_stream(side)
        for t in nxt:
            t.record_stream(torch.cuda.current_stream())
        losses.append(tr.train_step(*cur, next_pc=nxt[0], next_labels=nxt[1], next_smpw=nxt[2]))
        cur = nxt
    train.check_last()
    assert all(np.isfinite(losses)), losses
    assert int(aug.batch_counter.item()) == 4 and int(train.batch_counter.item()) == 4
