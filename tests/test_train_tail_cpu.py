"""CPU tests for the training step's elementwise tail (csrc/pn2_train.hip): the host model of the dropout draw that the GPU
tests use as their oracle is itself checked here, and the refusals that happen before any launch are pinned."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_ref as D  # noqa: E402

PN2_EINVAL, PN2_ERANGE, PN2_EUNSUP = -1, -3, -4


def test_error_codes_match_the_header(pn2):
    L = pn2._lib.lib
    assert b"PN2_EINVAL" in L.pn2_strerror(PN2_EINVAL)
    assert b"PN2_EUNSUP" in L.pn2_strerror(PN2_EUNSUP)
    assert b"PN2_ERANGE" in L.pn2_strerror(PN2_ERANGE)


def test_vectorised_draw_equals_the_plain_integer_form():
    for seed, step in [(77, 3), (9, 0), (-5, 1), (0x7FFFFFFF00000001, 2 ** 40), (D.KEEP_ONE_SEED, 0), (-2 ** 63, 2 ** 63 - 1)]:
        v = D.draws(seed, step, 10)
        assert v.dtype == np.uint32
        assert [int(a) for a in v] == [D.draw_int(seed, step, j) for j in range(10)]
        far = 2 ** 33 + 5  # an index past 32 bits, and the `start` argument
        assert [int(a) for a in D.draws(seed, step, 3, start=far)] == [D.draw_int(seed, step, far + j) for j in range(3)]
    assert D.threshold(0.5) == 1 << 31
    assert D.threshold(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32) == 429496736  # float32(0.1) = 0.100000001490116...
    assert D.threshold(0.9) == 3865470464


@pytest.mark.parametrize("keep", [0.1, 0.5, 0.9])
def test_keep_rate_within_four_binomial_sigma(keep):
    n = 1 << 24
    p = float(np.float32(keep))
    rate = D.keep_bits(9, 0, n, keep).mean()
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(rate - p) <= 4 * sigma, (rate, (rate - p) / sigma)


def test_steps_draw_independently():
    n = 1 << 24
    both = (D.keep_bits(9, 0, n, 0.5) & D.keep_bits(9, 1, n, 0.5)).mean()
    sigma = (0.25 * 0.75 / n) ** 0.5
    assert abs(both - 0.25) <= 4 * sigma, both


def test_mix_inverse_builds_the_seed_that_draws_all_ones():
    """The mix is a bijection: seed_for_output inverts it.  The constructed seed makes element 0 of step 0 draw 0xFFFFFFFF --
    the one draw that a bare `draw < 0xFFFFFFFF` rule drops at keep_prob = 1 -- and is negative as int64."""
    assert D.KEEP_ONE_SEED == 0xd6c7bb39feb8a004 - (1 << 64) and D.KEEP_ONE_SEED < 0
    assert D.mix64_int(D.KEEP_ONE_SEED, 0, 0) == D.KEEP_ONE_OUTPUT
    assert D.draw_int(D.KEEP_ONE_SEED, 0, 0) == 0xFFFFFFFF
    assert int(D.draws(D.KEEP_ONE_SEED, 0, 1)[0]) == 0xFFFFFFFF
    assert not (D.draws(D.KEEP_ONE_SEED, 0, 1)[0] < np.uint32(0xFFFFFFFF))  # the bare rule would drop element 0
    assert D.keep_bits(D.KEEP_ONE_SEED, 0, 1027, 1.0).all()                 # the model keeps everything at keep >= 1
    rs = np.random.RandomState(4)
    for _ in range(20):  # the inverse at other steps and indices
        out, step, i = (int(rs.randint(0, 2 ** 32)) << 32 | int(rs.randint(0, 2 ** 32)) for _ in range(3))
        seed = D.seed_for_output(out, step, i)
        assert -2 ** 63 <= seed < 2 ** 63 and D.mix64_int(seed, step, i) == out


def test_apply_scales_kept_elements_and_zeroes_the_rest():
    x = np.array([1.5, np.nan, np.inf, -0.0, 3.0], np.float32)
    y = D.apply(x, np.array([True, False, True, True, False]), 0.5)
    assert y.dtype == np.float32
    assert y.view(np.uint32).tolist() == np.array([3.0, 0.0, np.inf, -0.0, 0.0], np.float32).view(np.uint32).tolist()


def test_train_tail_refusals_need_no_gpu(pn2):
    L = pn2._lib.lib
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    nul = None
    assert L.pn2_weighted_ce_forward(16, 65, fake, fake, 0, fake, fake, fake, fake, nul) == PN2_EUNSUP
    assert L.pn2_weighted_ce_forward(16, 64, nul, fake, 0, fake, fake, fake, fake, nul) == -2  # 64 classes pass that check
    assert L.pn2_weighted_ce_forward(0, 9, fake, fake, 0, fake, fake, fake, fake, nul) == PN2_EINVAL
    assert L.pn2_weighted_ce_forward(0, 9, fake, fake, 1, fake, fake, fake, fake, nul) == PN2_EINVAL
    for keep in (0.0, -0.5, 1.0000001, 2.0, float("nan")):
        assert L.pn2_dropout(16, fake, keep, fake, fake, fake, nul) == PN2_EINVAL, keep
        assert L.pn2_dropout_grad(16, fake, fake, keep, fake, nul) == PN2_EINVAL, keep
    assert L.pn2_dropout(0, fake, 0.5, fake, fake, fake, nul) == PN2_EINVAL

    def tables(n):
        return (ctypes.c_void_p * n)(*[4096] * n), (ctypes.c_void_p * n)(*[8192] * n), (ctypes.c_uint64 * n)(*[16] * n)

    def fills(dsts, sizes):
        k = len(dsts)
        return k, (ctypes.c_void_p * k)(*dsts), (ctypes.c_uint64 * k)(*[1] * k), (ctypes.c_int * k)(*sizes)

    s, d, b = tables(49)
    assert L.pn2_multi_copy_fill(49, s, d, b, 0, nul, nul, nul, nul) == PN2_ERANGE
    assert L.pn2_multi_copy(49, s, d, b, nul) == PN2_ERANGE
    s, d, b = tables(2)
    assert L.pn2_multi_copy_fill(2, s, d, b, *fills([4096] * 5, [4] * 5), nul) == PN2_ERANGE
    assert L.pn2_multi_copy_fill(2, s, d, b, *fills([4096], [2]), nul) == PN2_EINVAL
    assert L.pn2_multi_copy_fill(2, s, d, b, *fills([4096, 4096], [4, 16]), nul) == PN2_EINVAL
    assert L.pn2_multi_copy_fill(2, s, d, b, *fills([4098], [4]), nul) == PN2_EINVAL        # 4-byte fill off a 4-byte boundary
    assert L.pn2_multi_copy_fill(2, s, d, b, *fills([4096, 4100], [4, 8]), nul) == PN2_EINVAL  # 8-byte fill on a 4-byte boundary
    assert L.pn2_multi_copy_fill(0, s, d, b, 0, nul, nul, nul, nul) == PN2_EINVAL
    assert L.pn2_multi_copy_fill(2, s, d, b, -1, nul, nul, nul, nul) == PN2_EINVAL
