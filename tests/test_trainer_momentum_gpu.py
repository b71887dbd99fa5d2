"""Trainer(optimizer="momentum") -- tf.train.MomentumOptimizer(lr, momentum=0.9), the other branch of the reference's
train.py:380-388 -- on the small model of test_train_gpu.test_captured_training_step_equals_eager: the first step against the
formula, every capture form against the eager run, the staged path and a learning-rate staircase that moves.  The device's
lr slot holds the PLAIN scheduled rate (no Adam bias correction) wherever it is written from."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import s_scene  # noqa: E402

pytestmark = pytest.mark.gpu

P_RTOL, P_ATOL = 2e-6, 2e-7  # the kernel tolerances of tests/test_momentum_gpu.py (test_adam_step_matches_tf_formula's)


def _hp(pn2, **extra):
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16, optimizer="momentum")
    hp.update(extra)
    return hp


def _batch(cuda, seed=0, b=8, n=2048):
    import torch
    rs = np.random.RandomState(seed)
    T = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    pc = T(np.concatenate([s_scene(seed + 1, b, n), rs.random_sample((b, n, 3)).astype(np.float32)], 2))
    return pc, T(rs.randint(0, 9, (b, n)).astype(np.int64)), T((rs.random_sample((b, n)) + 0.5).astype(np.float32))


@pytest.fixture(scope="module")
def batches(cuda):
    return [_batch(cuda, s) for s in range(3)]


def _trainer(pn2, cuda, hp, **kw):
    return pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=cuda, seed=3), **kw)


def _lr_slot(tr):
    import torch
    torch.cuda.synchronize()
    return float(tr.hyper[0])


def test_first_momentum_step_is_the_formula(pn2, cuda, batches):
    """one eager step from accum = 0: accum == g * grad_scale bit for bit (0.9 * 0 + g'), p_after = p_before - lr * accum, with g
    the step's gradient as it lies in the trainer's flat gradient buffer (it is zero-filled only by the next step)"""
    import torch
    tr = _trainer(pn2, cuda, _hp(pn2), capture=False)
    tr._lazy_init(batches[0][0])
    assert tr.optimizer == "momentum" and tr.flat_v is None and tr.flat_m is None, "no second-moment buffer"
    assert list(tr.slots) == ["accum"] and tr.flat_accum.shape == tr.flat_p.shape and float(tr.flat_accum.abs().max()) == 0.0
    assert tr.hyper.numel() == 3 and tr._lr_slot.data_ptr() == tr.hyper.data_ptr()
    p_before = tr.flat_p.clone()
    loss = tr.train_step(*batches[0])
    torch.cuda.synchronize()
    assert np.isfinite(loss) and tr.step_count == 1
    lr = pn2.train.learning_rate(0, 8)
    hyper = tr.hyper.cpu().numpy()
    assert hyper[0] == np.float32(lr) and lr == 1e-3, "the lr slot holds the plain scheduled rate"
    assert hyper[0] != np.float32(pn2.train.adam_lr_t(lr, 1))
    np.testing.assert_array_equal(hyper[1:], np.array([0.9, 1.0], np.float32))
    g = tr.bucket.flat.clone()
    assert float(g.abs().max()) > 0 and g.numel() == tr.flat_p.numel()
    assert torch.equal(tr.flat_accum, g * float(hyper[2]))
    want = p_before.double().cpu().numpy() - float(hyper[0]) * tr.flat_accum.double().cpu().numpy()
    np.testing.assert_allclose(tr.flat_p.cpu().numpy(), want, rtol=P_RTOL, atol=P_ATOL)
    assert float((tr.flat_p - p_before).abs().max()) > 0


def test_every_capture_form_follows_the_eager_momentum_run(pn2, cuda, batches):
    """eager, a second eager run (the noise of the gradient kernels' fp32 atomics), the single graph, the split capture and the
    three-segment capture, seven steps each: the yardstick and both numbers are test_captured_training_step_equals_eager's.
    Then five run-ahead steps: the device scalars are [lr of the last step, 0.9, 1.0]."""
    import torch
    hp = _hp(pn2)
    out = {}
    for key, capture in (("eager", False), ("eager2", False), ("graph", True), ("split", True), ("split3", True)):
        tr = _trainer(pn2, cuda, hp, capture=capture, warmup_eager=2, split_capture=key.startswith("split"),
                      overlap_collective=(key == "split3"))
        losses = [tr.train_step(*batches[i % 3]) for i in range(7)]
        assert (tr._graph is not None) == capture and (tr._graph_adam is not None) == key.startswith("split")
        assert (tr._graph_late is not None) == (key == "split3")
        assert tr.step_count == 7 and all(np.isfinite(losses)) and tr.flat_v is None
        out[key] = (losses, tr.flat_p.clone(), tr)
    dist = lambda a, b: float((out[a][1] - out[b][1]).norm() / out[b][1].norm())  # noqa: E731
    noise = dist("eager2", "eager")
    for key in ("graph", "split", "split3"):
        print("momentum %s: distance to eager %.3g, eager-to-eager noise %.3g" % (key, dist(key, "eager"), noise))
        assert dist(key, "eager") <= 3.0 * noise + 2e-2, (key, dist(key, "eager"), noise)
        np.testing.assert_allclose(out[key][0], out["eager"][0], rtol=3e-2)
    for key in ("graph", "split", "split3"):
        tr = out[key][2]
        for i in range(7, 12):
            tr.train_step(*batches[i % 3], sync=False)
        torch.cuda.synchronize()
        want = [pn2.train.learning_rate(11, 8), 0.9, 1.0]
        np.testing.assert_allclose(tr.hyper.cpu().numpy(), want, rtol=1e-6)


def test_staged_momentum_steps_write_the_plain_rate(pn2, cuda, batches):
    """the whole next batch announced on every call (test_staged_next_batch_steps_with_graphs_only): the geometry stream stages
    the next step's lr; decay_step = 16 makes that rate change every two steps, so a staged Adam-style or stale value shows"""
    hp = _hp(pn2, decay_step=16)
    tr = _trainer(pn2, cuda, hp, capture=True, warmup_eager=2)
    staged = []
    for i in range(9):
        nb = batches[(i + 1) % 3]
        staged.append(tr._staged_tag is not None)
        loss = tr.train_step(*batches[i % 3], next_pc=nb[0], next_labels=nb[1], next_smpw=nb[2])
        assert np.isfinite(loss)
        want = pn2.train.learning_rate(i, 8, decay_step=16)
        np.testing.assert_allclose(_lr_slot(tr), want, rtol=1e-6, err_msg="step %d" % i)
    # steps 0, 1 are eager, 2 captures; the batch-norm decay moves with the staircase, so some later steps recapture (and copy)
    # instead of taking the staged batch -- but staged steps there are
    assert tr._copy_graph is not None and tr._staging is not None and any(staged[3:]), staged
    assert pn2.train.learning_rate(8, 8, decay_step=16) < 0.3e-3


def test_staged_momentum_steps_constant_schedule(pn2, cuda, batches):
    """the same with the reference's decay_step (no recapture): from step 3 on every batch was staged by the step before, and the
    lr slot read back after each step is the plain scheduled rate of that step"""
    tr = _trainer(pn2, cuda, _hp(pn2), capture=True, warmup_eager=2)
    staged = []
    for i in range(7):
        nb = batches[(i + 1) % 3]
        staged.append(tr._staged_tag is not None)
        assert np.isfinite(tr.train_step(*batches[i % 3], next_pc=nb[0], next_labels=nb[1], next_smpw=nb[2]))
        np.testing.assert_allclose(_lr_slot(tr), pn2.train.learning_rate(i, 8), rtol=1e-6, err_msg="step %d" % i)
    assert all(staged[3:]) and not any(staged[:3]), staged


def test_momentum_follows_a_learning_rate_staircase(pn2, cuda, batches):
    """decay_step = 16: the staircase drops every two steps at B = 8.  Eager and captured runs of six steps: the lr slot after
    each step is learning_rate(step, 8, decay_step=16), and both runs end within the yardstick of each other."""
    hp = _hp(pn2, decay_step=16)
    out = {}
    for key, capture in (("eager", False), ("eager2", False), ("graph", True)):
        tr = _trainer(pn2, cuda, hp, capture=capture, warmup_eager=2)
        rates = []
        for i in range(6):
            assert np.isfinite(tr.train_step(*batches[i % 3]))
            rates.append(_lr_slot(tr))
        want = [pn2.train.learning_rate(i, 8, decay_step=16) for i in range(6)]
        assert want[0] == 1e-3 and want[2] < want[1] == want[0] and want[4] < want[3] == want[2]
        np.testing.assert_allclose(rates, want, rtol=1e-6, err_msg=key)
        assert (tr._graph is not None) == capture
        out[key] = tr.flat_p.clone()
    dist = lambda a, b: float((out[a] - out[b]).norm() / out[b].norm())  # noqa: E731
    noise = dist("eager2", "eager")
    print("momentum staircase: graph to eager %.3g, eager-to-eager noise %.3g" % (dist("graph", "eager"), noise))
    assert dist("graph", "eager") <= 3.0 * noise + 2e-2, (dist("graph", "eager"), noise)
