"""The momentum optimizer at the drop-in boundary, without a GPU: pn2_momentum_step is exported and refuses bad arguments before
any launch, and Trainer accepts the reference's two optimizer names (train.py:380-388) and nothing else."""
import ctypes

import pytest

PN2_EINVAL, PN2_ENULL = -1, -2


def test_momentum_step_is_exported(pn2):
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    assert hasattr(lib, "pn2_momentum_step")
    assert "pn2_momentum_step" in pn2._lib.SIGNATURES
    assert "pn2_momentum_step" in pn2._lib._STATEFUL  # it updates its inputs in place: the dup hook must not launch it twice


def test_momentum_step_argument_checks_need_no_gpu(pn2):
    L = pn2._lib.lib
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    for n in (0, -1):
        assert L.pn2_momentum_step(n, fake, fake, fake, fake, None) == PN2_EINVAL
    for at in range(4):  # params, grads, accum, hyper in turn
        args = [fake] * 4
        args[at] = None
        assert L.pn2_momentum_step(16, *args, None) == PN2_ENULL, at
    assert L.pn2_momentum_step(0, None, None, None, None, None) == PN2_EINVAL  # the size is looked at first, as pn2_adam_step does


def test_trainer_accepts_adam_and_momentum_only(pn2):
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    store = pn2.util.tf_util.VariableStore(device="cpu", seed=0)
    tr = pn2.train.Trainer({**hp, "optimizer": "momentum"}, 9, store=store, device="cpu")
    assert tr.optimizer == "momentum" and tr.momentum == hp["momentum"] == 0.9
    assert pn2.train.Trainer({**hp, "optimizer": "MOMENTUM"}, 9, store=store, device="cpu").optimizer == "momentum"
    assert pn2.train.Trainer({**hp, "optimizer": "momentum", "momentum": 0.5}, 9, store=store, device="cpu").momentum == 0.5
    no_key = {k: v for k, v in hp.items() if k != "momentum"}
    assert pn2.train.Trainer({**no_key, "optimizer": "momentum"}, 9, store=store, device="cpu").momentum == 0.9
    assert pn2.train.Trainer(hp, 9, store=store, device="cpu").optimizer == "adam"
    with pytest.raises(ValueError, match="sgd"):
        pn2.train.Trainer({**hp, "optimizer": "sgd"}, 9, store=store, device="cpu")


def test_state_is_refused_before_any_variable_exists(pn2):
    """the two things a fresh trainer can say without a batch: another optimizer's state is refused at once, and there is no
    state to give yet"""
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    store = pn2.util.tf_util.VariableStore(device="cpu", seed=0)
    tr = pn2.train.Trainer(hp, 9, store=store, device="cpu")
    with pytest.raises(ValueError, match="momentum"):
        tr.load_state_dict({"variables": {}, "optimizer": {"name": "momentum", "slots": {}}, "step_count": 3, "dropout_seeds": {}})
    assert tr._pending_state is None and tr.step_count == 0
    with pytest.raises(RuntimeError, match="no variables yet"):
        tr.state_dict()
