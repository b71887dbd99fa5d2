"""The host model of the batch-norm kernels (tests/bn_ref.py) checked by itself: its float64 gradient against torch's float64
autograd, its float32 tie / ysel rule on a group made by hand, its tolerance helper on a case with a known answer, and the
input of the GPU cancellation test (tests/test_bn_edges_gpu.py) shown to be fair to a float64 one-pass variance and fatal to a
float32 one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as B  # noqa: E402


def _case(groups, pool, c, seed):
    rs = np.random.RandomState(seed)
    p = max(pool, 1)
    y = rs.randn(groups, p, c)
    if pool > 1:
        y[::2, p // 2:, :] = y[::2, :1, :]      # the second half of every other group repeats its first row: exact ties
        y[1, :, :] = y[1, :1, :]                # a group of identical rows
    else:
        y[1::3] = y[0]                          # repeated rows
    y = y.reshape(groups * p, c)
    gamma, beta = 0.5 + rs.rand(c), rs.randn(c) * 0.3
    beta[0] = -6.0                              # a channel that never passes the ReLU: every row ties at 0
    return y, gamma, beta, rs.randn(groups, c)


@pytest.mark.parametrize("groups,pool,c", [(12, 0, 3), (5, 4, 6), (4, 3, 5)])
@pytest.mark.parametrize("relu", [0, 1])
def test_float64_gradient_equals_torch_autograd(oracle, groups, pool, c, relu):
    """bn_ref.forward64 / backward64 (the oracle's batch norm, ReLU and max over groups of rows, with duplicated rows, a group of
    identical rows and a channel dead under the ReLU) against F.batch_norm(training=True) + relu + amax in float64 autograd:
    z, dy, dgamma, dbeta within 1e-12 of the output scale."""
    import torch
    import torch.nn.functional as Fn
    y, gamma, beta, dz = _case(groups, pool, c, 7 * groups + pool)
    eps = 1e-3
    fw = B.forward64(oracle, y, gamma, beta, relu, eps, pool)
    dy, dg, db = B.backward64(oracle, y, gamma, beta, dz, relu, eps, pool, z_pattern=fw["z"])
    ty, tg, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (y, gamma, beta))
    tz = Fn.batch_norm(ty, None, None, tg, tb, training=True, eps=eps)
    if relu:
        tz = torch.relu(tz)
    out = tz.reshape(groups, pool, c).amax(dim=1) if pool > 1 else tz
    out.backward(torch.tensor(dz, dtype=torch.float64))
    ref_out = fw["zmax"] if pool > 1 else fw["z"]
    for got, ref in ((ref_out, out.detach().numpy()), (dy, ty.grad.numpy()), (dg, tg.grad.numpy()), (db, tb.grad.numpy())):
        assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
    if pool > 1:
        assert fw["ties"].max() >= pool - pool // 2 + 1 and (not relu or (fw["ties"][:, 0] == pool).all())


def test_restated_ties_and_ysel_on_a_group_made_by_hand():
    """one group of 5 rows, identity normalisation (gamma = 1, beta = +-0, mean = 0, invstd = 1): the maximum, how many rows attain
    it, and ysel = the y of the FIRST of them -- including a channel whose rows are -0 and +0 (equal, so all tie, and the pooled
    value keeps the first row's sign bit) and, under the ReLU, a channel of negative values that ties at 0 on every row"""
    y = np.array([[1.0, -0.0, -3.0, 2.0],
                  [4.0, 0.0, -1.0, 2.0],
                  [4.0, -0.0, -2.0, 1.0],
                  [2.0, 0.0, -1.0, 2.0],
                  [4.0, 0.0, -5.0, 0.5]], np.float32)
    one, zero = np.ones(4, np.float32), np.zeros(4, np.float32)
    beta = np.array([0.0, -0.0, 0.0, 0.0], np.float32)   # sh = fma(-0, 1, -0) = -0 in channel 1: fma(y, 1, sh) keeps the sign of a zero y
    r = B.restate(y, one, beta, 0, zero, one, dz=np.array([[3.0, 1.0, 1.0, 6.0]], np.float32), pool=5)
    assert np.array_equal(r["zmax"], [[4.0, 0.0, -1.0, 2.0]]) and np.signbit(r["zmax"][0, 1])
    assert np.array_equal(r["ties"], [[3.0, 5.0, 2.0, 3.0]])
    assert np.array_equal(r["ysel"], [[4.0, 0.0, -1.0, 2.0]]) and np.signbit(r["ysel"][0, 1])
    assert np.array_equal(r["g"][:, 0], [0, 1, 1, 0, 1]) and np.array_equal(r["g"][:, 3], [2, 2, 0, 2, 0])
    assert np.array_equal(r["g"][:, 1], np.full(5, np.float32(1) / np.float32(5)))
    assert np.array_equal(r["dbeta"], [3.0, 1.0, 1.0, 6.0]) and np.array_equal(r["dbetap"], [3.0, 1.0, 1.0, 6.0])
    assert np.array_equal(r["dgamma"], [12.0, 0.0, -1.0, 12.0]) and np.array_equal(r["dgammap"], r["dgamma"])
    r = B.restate(y, one, beta, 1, zero, one, dz=np.array([[3.0, 1.0, 1.0, 6.0]], np.float32), pool=5)
    assert np.array_equal(r["zmax"], [[4.0, 0.0, 0.0, 2.0]]) and not np.signbit(r["zmax"][0, 1:3]).any()
    assert np.array_equal(r["ties"], [[3.0, 5.0, 5.0, 3.0]])
    assert np.array_equal(r["ysel"], [[4.0, 0.0, -3.0, 2.0]])          # channel 2: the first row, although it is not the largest y
    assert np.array_equal(r["dbeta"], [3.0, 0.0, 0.0, 6.0]) and np.array_equal(r["dbetap"], r["dbeta"])   # the floor passes nothing


def test_bound_helper_on_a_known_case():
    """reference (1, 2, 1024) restated as (1, 2 + 2^-20, 1024 - 2^-13): measured 2^-13, bound 4 x that; an exact restatement is
    floored at 1 float32 ulp of the scale (2^-13 at 1024); per channel the measured figure is taken by column; a non-finite
    reference entry is left out"""
    ref = np.array([1.0, 2.0, 1024.0])
    b, m = B.bound(np.array([1.0, 2.0 + 2.0 ** -20, 1024.0 - 2.0 ** -13]), ref)
    assert m == 2.0 ** -13 and b == 2.0 ** -11
    b, m = B.bound(ref.astype(np.float32), ref)
    assert m == 0.0 and b == 2.0 ** -13
    ref2 = np.array([[1.0, 8.0], [3.0, -1024.0]])
    b, m = B.bound(np.array([[1.5, 8.0], [3.0, -1024.0]]), ref2, per_channel=True)
    assert np.array_equal(m, [0.5, 0.0]) and np.array_equal(b, [2.0, 2.0 ** -13])
    b, m = B.bound(np.array([1.0, np.nan]), np.array([1.0, np.inf]))
    assert m == 0.0 and b == 2.0 ** -23
    assert np.array_equal(B.ulps(np.float32(1) + np.float32(2.0 ** -22), 1.0), 2.0)


def _pairwise(v):
    return v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:])


def test_cancellation_input_is_fair_to_float64_and_fatal_to_float32():
    """The GPU cancellation test's input (5000 rows of 64 + 0.05 * randn, eps = 1e-3).  invstd from the ONE-PASS formula
    E[y^2] - E[y]^2 with float64 sums taken in four orders -- sequential, reversed, pairwise, 512-row slabs then added -- stays
    within 1 float32 ulp of the exact two-pass value (math.fsum): measured worst 0.054 ulp.  The same formula with float32
    sums misses it by more than 100 ulp: measured, best of the 8 channels, 2.9e6 ulp.  So the 2-ulp bound of the GPU test is met by a float64
    accumulator in any summation order and by no float32 one."""
    y = B.cancellation_input()
    rows, eps = y.shape[0], 1e-3
    worst64, best32 = 0.0, np.inf
    for ch in range(y.shape[1]):
        mean, var = B.moments_two_pass(y[:, ch])
        exact = 1.0 / np.sqrt(var + eps)
        d = y[:, ch].astype(np.float64)
        orders = {"sequential": lambda v: np.cumsum(v)[-1], "reversed": lambda v: np.cumsum(v[::-1])[-1],
                  "pairwise": lambda v: _pairwise(list(v)),
                  "slabs": lambda v: np.cumsum([np.cumsum(v[i:i + 512])[-1] for i in range(0, rows, 512)])[-1]}
        for name, total in orders.items():
            m = total(d) / rows
            inv = 1.0 / np.sqrt(max(total(d * d) / rows - m * m, 0.0) + eps)
            worst64 = max(worst64, float(B.ulps(inv, exact)))
        s = y[:, ch]
        m32 = np.cumsum(s, dtype=np.float32)[-1] / np.float32(rows)
        v32 = np.cumsum(s * s, dtype=np.float32)[-1] / np.float32(rows) - m32 * m32
        inv32 = np.float32(1) / np.sqrt(np.maximum(v32, np.float32(0)) + np.float32(eps))
        best32 = min(best32, float(B.ulps(inv32, exact)))
    print("float64 one-pass, four orders: worst %.2g ulp; float32 one-pass: best channel %.3g ulp" % (worst64, best32))
    assert worst64 < 1.0
    assert best32 > 100.0
