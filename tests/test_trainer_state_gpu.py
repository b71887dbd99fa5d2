"""Stop and continue: Trainer.state_dict / load_state_dict / save / load for both optimizers, on the small model of
test_train_gpu.test_captured_training_step_equals_eager.  The saved state names the optimizer's slots by variable and carries
the step count (learning-rate staircase, batch-norm decay, Adam's bias correction, dropout stream) and the dropout seeds.

Two runs of the same steps differ by the order of the gradient kernels' fp32 atomics, so wherever a continued run is held
against the uninterrupted one the yardstick is a second uninterrupted run (3 x its distance + 2e-2, the numbers of
test_captured_training_step_equals_eager); what a load must reproduce exactly -- the file itself, the inference logits computed
from it -- is compared with torch.equal."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import s_scene  # noqa: E402

pytestmark = pytest.mark.gpu

SLOTS = {"adam": ("m", "v"), "momentum": ("accum",)}


def _hp(pn2, optimizer):
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16, optimizer=optimizer)
    return hp


def _batch(cuda, seed=0, b=8, n=2048):
    import torch
    rs = np.random.RandomState(seed)
    T = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    pc = T(np.concatenate([s_scene(seed + 1, b, n), rs.random_sample((b, n, 3)).astype(np.float32)], 2))
    return pc, T(rs.randint(0, 9, (b, n)).astype(np.int64)), T((rs.random_sample((b, n)) + 0.5).astype(np.float32))


@pytest.fixture(scope="module")
def batches(cuda):
    return [_batch(cuda, s) for s in range(4)]  # three to train on, batches[3] to evaluate on


def _trainer(pn2, cuda, optimizer, seed=3, **kw):
    kw.setdefault("warmup_eager", 2)
    return pn2.train.Trainer(_hp(pn2, optimizer), 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=seed), **kw)


def _eval_logits(tr, batch):
    import torch
    tr.eval_step(*batch)
    torch.cuda.synchronize()
    return tr.last_eval_logits.clone()


def assert_same_state(a, b):
    import torch
    assert a["optimizer"]["name"] == b["optimizer"]["name"] and a["step_count"] == b["step_count"]
    assert a["dropout_seeds"] == b["dropout_seeds"]
    for part in (lambda s: s["variables"], lambda s: s["optimizer"]["slots"]):
        assert list(part(a)) == list(part(b))
        for k, v in part(a).items():
            assert not v.is_cuda and not part(b)[k].is_cuda
            assert torch.equal(v, part(b)[k]), k


def _final(tr):
    import torch
    torch.cuda.synchronize()
    return {"p": tr.flat_p.clone(), "b": torch.cat([tr.store.buffers[k].flatten() for k in sorted(tr.store.buffers)]),
            "lr": float(tr.hyper[0]), "steps": tr.step_count}


@pytest.fixture(scope="module", params=["adam", "momentum"])
def runs(request, pn2, cuda, batches, tmp_path_factory):
    """shared by the tests below, computed once per optimizer: run A of seven steps (two eager, the capture, replays) whose state
    is taken -- and saved to a file -- after step four, with its inference logits on batches[3] at that point, and a second
    uninterrupted run A2 of the same steps (the noise)"""
    opt = request.param
    path = str(tmp_path_factory.mktemp("state") / ("trainer_%s.pt" % opt))
    a = _trainer(pn2, cuda, opt)
    for i in range(4):
        a.train_step(*batches[i % 3])
    assert a._graph is not None
    state4 = a.state_dict()
    a.save(path)
    logits4 = _eval_logits(a, batches[3])
    for i in range(4, 7):
        a.train_step(*batches[i % 3])
    a2 = _trainer(pn2, cuda, opt)
    for i in range(7):
        a2.train_step(*batches[i % 3])
    return {"opt": opt, "path": path, "state4": state4, "logits4": logits4, "a": _final(a), "a2": _final(a2)}


def test_state_dict_layout(pn2, runs):
    """plain containers of CPU tensors and Python scalars; slots by variable name; the file holds the same"""
    import torch
    st, opt = runs["state4"], runs["opt"]
    assert set(st) == {"variables", "optimizer", "step_count", "dropout_seeds"} and st["step_count"] == 4
    assert st["optimizer"]["name"] == opt and isinstance(st["step_count"], int)
    names = [k for k in st["variables"] if not k.endswith(("moving_mean", "moving_variance"))]
    assert len(names) < len(st["variables"]), "moving averages are part of the variables"
    assert set(st["optimizer"]["slots"]) == {"%s/%s" % (k, s) for k in names for s in SLOTS[opt]}
    for k in names:
        for s in SLOTS[opt]:
            assert st["optimizer"]["slots"]["%s/%s" % (k, s)].shape == st["variables"][k].shape
    assert st["dropout_seeds"] and all(isinstance(v, int) for v in st["dropout_seeds"].values())
    moved = sum(float(v.abs().sum()) for v in st["optimizer"]["slots"].values())
    assert moved > 0, "four steps left the slots at zero"
    assert_same_state(torch.load(runs["path"], weights_only=True, map_location="cpu"), st)


def test_round_trip_through_a_file(pn2, cuda, batches, runs):
    """the file into a fresh trainer B, which then steps; and into a fresh trainer C, whose inference logits on a fixed batch equal
    A's right after the save and whose own state_dict() is the file, tensor for tensor"""
    import torch
    opt = runs["opt"]
    b = _trainer(pn2, cuda, opt)
    b.load(runs["path"])
    assert b.bucket is None and b.step_count == 0  # nothing exists yet: applied when the first batch creates the variables
    loss = b.train_step(*batches[4 % 3])
    assert np.isfinite(loss) and b.step_count == 5 and b._graph is None  # a resumed trainer warms up eagerly, too
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(b.hyper[0]), b._optimizer_lr(4, 8), rtol=1e-6)  # Adam: the bias correction of t = 5
    for t in b.store._dropout.values():
        assert int(t[1]) == 4
    c = _trainer(pn2, cuda, opt)
    c.load(runs["path"])
    logits = _eval_logits(c, batches[3])
    assert torch.equal(logits, runs["logits4"]), float((logits - runs["logits4"]).abs().max())
    assert c.step_count == 4
    assert_same_state(c.state_dict(), torch.load(runs["path"], weights_only=True, map_location="cpu"))
    assert_same_state(c.state_dict(), runs["state4"])


def test_continued_run_follows_the_uninterrupted_one(pn2, cuda, batches, runs):
    """B' loads A's state of step four and runs steps five to seven on the same batches (two eager, then its own capture)"""
    opt = runs["opt"]
    bp = _trainer(pn2, cuda, opt)
    bp.load_state_dict(runs["state4"])
    for i in range(4, 7):
        assert np.isfinite(bp.train_step(*batches[i % 3]))
    assert bp._graph is not None
    got, a, a2 = _final(bp), runs["a"], runs["a2"]
    assert got["steps"] == 7 == a["steps"]
    assert got["lr"] == a["lr"]
    for key in ("p", "b"):
        dist = lambda x, y: float((x[key] - y[key]).norm() / y[key].norm())  # noqa: E731
        noise = dist(a2, a)
        print("%s continued run, %s: distance to the uninterrupted run %.3g, noise %.3g" % (opt, key, dist(got, a), noise))
        assert dist(got, a) <= 3.0 * noise + 2e-2, (key, dist(got, a), noise)


def test_in_place_load_on_a_live_trainer(pn2, cuda, batches, runs):
    """a captured trainer goes back to its own state of step four: no buffer moves (the graphs hold raw addresses), the graph is
    kept and replayed, and the folded inference weights are rebuilt"""
    import torch
    opt = runs["opt"]
    a = _trainer(pn2, cuda, opt)
    for i in range(4):
        a.train_step(*batches[i % 3])
    state = a.state_dict()
    nb = batches[6 % 3]
    a.train_step(*batches[4 % 3])
    a.train_step(*batches[5 % 3], next_pc=nb[0], next_labels=nb[1], next_smpw=nb[2])  # leaves a staged batch behind
    assert a._staged_tag is not None
    stale = _eval_logits(a, batches[3])  # fills the folded-weight cache from the step-six weights
    ptrs = [a.flat_p.data_ptr()] + [t.data_ptr() for t in a.slots.values()] + [a.hyper.data_ptr()]
    graph, epoch = a._graph, a.store.train_epoch
    a.load_state_dict(state)
    assert ptrs == [a.flat_p.data_ptr()] + [t.data_ptr() for t in a.slots.values()] + [a.hyper.data_ptr()]
    assert a.step_count == 4 and a._graph is graph and a.store.train_epoch > epoch
    assert a._geo is None and a._geo_tag is None and a._staged_tag is None
    assert_same_state(a.state_dict(), state)
    for p in a.store.parameters():  # still views of the flat buffer
        assert a.flat_p.data_ptr() <= p.data_ptr() < a.flat_p.data_ptr() + 4 * a.flat_p.numel()
    warm = _eval_logits(a, batches[3])
    a.store._folded.clear()  # what a cold cache computes from the loaded parameters and moving averages
    a.store.train_epoch += 1
    cold = _eval_logits(a, batches[3])
    assert torch.equal(warm, cold), float((warm - cold).abs().max())
    assert float((warm - stale).abs().max()) > 0, "the evaluation after the load served the weights from before it"
    loss = a.train_step(*batches[4 % 3])
    assert np.isfinite(loss) and a._graph is graph and a.step_count == 5, "the step after the load recaptured"
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(a.hyper[0]), a._optimizer_lr(4, 8), rtol=1e-6)


def test_states_that_do_not_fit_are_refused(pn2, cuda, batches):
    """ValueError, and the target's own state_dict() is what it was: another optimizer's state, a variable missing, a slot of another
    shape, a store built with another seed.  (Trainers whose variables exist but that have not stepped: _lazy_init.)"""
    import torch
    pc = batches[0][0]
    target = _trainer(pn2, cuda, "adam")
    target._lazy_init(pc)
    target.flat_m.fill_(0.25)  # something a half-done load would overwrite
    before = target.state_dict()
    good = copy.deepcopy(before)
    good["step_count"] = 9

    mom = _trainer(pn2, cuda, "momentum")
    mom._lazy_init(pc)
    other_seed = _trainer(pn2, cuda, "adam", seed=4)
    other_seed._lazy_init(pc)

    no_var = copy.deepcopy(good)
    del no_var["variables"][next(reversed(no_var["variables"]))]
    no_slot = copy.deepcopy(good)
    del no_slot["optimizer"]["slots"][next(iter(no_slot["optimizer"]["slots"]))]
    reshaped = copy.deepcopy(good)
    k = next(k for k, v in reshaped["optimizer"]["slots"].items() if v.numel() > 1)
    reshaped["optimizer"]["slots"][k] = reshaped["optimizer"]["slots"][k].flatten()[:-1].clone()
    reshaped_var = copy.deepcopy(good)
    k = next(k for k, v in reshaped_var["variables"].items() if v.dim() == 1 and v.numel() > 1)
    reshaped_var["variables"][k] = reshaped_var["variables"][k][:-1].clone()
    for what, state in (("momentum state into Adam", mom.state_dict()), ("variable removed", no_var), ("slot removed", no_slot),
                        ("slot of another shape", reshaped), ("variable of another shape", reshaped_var),
                        ("another seed", other_seed.state_dict())):
        with pytest.raises(ValueError):
            target.load_state_dict(state)
        assert_same_state(target.state_dict(), before)
        assert target.step_count == 0, what
    with pytest.raises(ValueError):
        mom.load_state_dict(good)
    # the seed is checked by the dropout seed words, not by the weights: the other store's weights do differ
    assert other_seed.state_dict()["dropout_seeds"] != before["dropout_seeds"]
    # a fresh trainer cannot know its variables or seeds before its first batch: it refuses when that batch creates them
    fresh = _trainer(pn2, cuda, "adam", seed=4)
    fresh.load_state_dict(good)
    with pytest.raises(ValueError):
        fresh._lazy_init(pc)
    assert fresh.step_count == 0 and fresh._pending_state is None
    # ... and the state that does fit loads
    target.load_state_dict(good)
    assert target.step_count == 9 and float(target.flat_m.min()) == 0.25
    torch.cuda.synchronize()
