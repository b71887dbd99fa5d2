"""Host model of the training-mode batch-norm kernels (csrc/pn2_bn.hip, pn2_bn_finish in csrc/pn2_common.h), numpy only.

Three parts:
  1. the float64 reference: oracle.batch_norm_relu_train / _grad and oracle.max_pool_rows / _grad, reused as they are
     (`forward64`, `backward64` only route arguments to them);
  2. the float32 restatement of the kernels' element formulas FROM SAVED MOMENTS -- sc = fl(gamma * invstd),
     sh = fl(fma(-mean, sc, beta)), z = fl(fma(y, sc, sh)), ReLU as t > 0 ? t : 0, the pooled maximum with its tie count and
     ysel (the y of the first row attaining it), and the gradient element sc * fma(-xh, k2, gk - k1) with
     xh = fl(fl(y - mu) * is).  An fma is a float64 product and sum rounded once to float32 (the product of two float32 is
     exact in float64).  The per-channel sums are float64 sums of those float32 elements, as in the kernels;
  3. `bound`: how far a float32 result may be from the float64 reference -- 4 x the error of the restatement (2) against the
     reference (1) on the same input, floored at 1 float32 ulp of the output scale.  It also returns the measured figure.
"""
import numpy as np

F32 = np.float32


def f32(a):
    """round float64 values to float32 once"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float64).astype(F32)


def fma32(a, b, c):
    """fl32(a * b + c) for float32 operands"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
                + np.asarray(c, F32).astype(np.float64)).astype(F32)


def ulp32(x):
    """spacing of float32 at |x| (float64 array)"""
    return np.spacing(np.abs(f32(x))).astype(np.float64)


def ulps(got, ref64):
    """|got - ref| in float32 ulps of ref, elementwise"""
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64)) / ulp32(ref64)


# ---------------------------------------------------------------------------------------------------- 1. float64 reference
def forward64(O, y, gamma, beta, relu, eps, pool=0, bias=None, moving=None, decay=0.9):
    """-> dict(z, mean, var, invstd[, zmax, ties][, mm, mv]) from the oracle"""
    with np.errstate(all="ignore"):
        out = O.batch_norm_relu_train(y, gamma, beta, bool(relu), eps, bias, moving, decay)
    r = dict(z=out[0], mean=out[1], var=out[2], invstd=1.0 / np.sqrt(out[2] + eps))
    if moving is not None:
        r["mm"], r["mv"] = out[3], out[4]
    if pool > 1:
        r["zmax"], r["ties"] = O.max_pool_rows(r["z"], pool)
    return r


def backward64(O, y, gamma, beta, dz, relu, eps, pool=0, z_pattern=None):
    """-> (dy, dgamma, dbeta) from the oracle.  z_pattern: a float32 implementation's forward value; it decides the ReLU mask
    (elements within rounding of zero) and, behind the max pool, which rows of a group tie for the maximum."""
    mask = None if z_pattern is None else np.asarray(z_pattern) > 0
    if pool > 1:
        dz = O.max_pool_rows_grad(z_pattern, pool, dz)
    with np.errstate(all="ignore"):
        return O.batch_norm_relu_train_grad(y, gamma, beta, dz, bool(relu), eps, mask=mask)


# ------------------------------------------------------------------------------------------------ 2. float32 restatement
def scale_shift32(gamma, beta, mean32, invstd32):
    with np.errstate(over="ignore", invalid="ignore"):
        sc = np.asarray(gamma, F32) * np.asarray(invstd32, F32)
    return sc, fma32(-np.asarray(mean32, F32), sc, beta)


def apply32(y, sc, sh, relu):
    """-> (z, on): z = relu?(fma(y, sc, sh)), on = the element passes the ReLU"""
    t = fma32(y, sc, sh)
    if not relu:
        return t, np.ones(t.shape, bool)
    with np.errstate(invalid="ignore"):
        on = t > 0
    return np.where(on, t, F32(0)), on


def pool32(z32, y, pool):
    """-> (zmax, ties, ysel) over groups of `pool` consecutive rows: the value of the FIRST row attaining the maximum (so a
    group of -0 and +0 keeps the bits of its first row), how many rows attain it, and that first row's y"""
    g = np.asarray(z32, F32).reshape(-1, pool, z32.shape[1])
    gy = np.asarray(y, F32).reshape(g.shape)
    sel = g == g.max(axis=1, keepdims=True)
    first = sel.argmax(axis=1)[:, None, :]
    return (np.take_along_axis(g, first, 1)[:, 0, :], sel.sum(axis=1).astype(F32), np.take_along_axis(gy, first, 1)[:, 0, :])


def incoming32(z32, pool, zmax, ties, dzp):
    """gradient reaching the un-pooled activation: fl(dzp / ties) on the rows that attain the maximum, 0 elsewhere"""
    g = np.asarray(z32, F32).reshape(-1, pool, z32.shape[1])
    with np.errstate(all="ignore"):
        share = np.asarray(dzp, F32) / np.asarray(ties, F32)
    return np.where(g == np.asarray(zmax, F32)[:, None, :], share[:, None, :], F32(0)).reshape(z32.shape).astype(F32)


def xhat32(y, mean32, invstd32):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(y, F32) - np.asarray(mean32, F32)) * np.asarray(invstd32, F32)


def grad_sums(y, g32, on, mean32, invstd32):
    """-> (sum gd, sum gd * xh) per channel in float64, gd = on ? g : 0 (bn_grad_reduce_kernel)"""
    gd = np.where(on, np.asarray(g32, F32), F32(0)).astype(np.float64)
    with np.errstate(all="ignore"):
        return gd.sum(axis=0), (gd * xhat32(y, mean32, invstd32).astype(np.float64)).sum(axis=0)


def grad_sums_pooled(dzp, zmax, ysel, relu, mean32, invstd32):
    """the same two sums from the pooled tensors alone (bn_grad_reduce_pooled_kernel): a group passes dzp whole -- n * fl(dzp / n)
    of the row-wise form becomes dzp -- at xh of ysel, unless its maximum is the ReLU's 0"""
    with np.errstate(all="ignore"):
        gd = np.where((np.asarray(zmax, F32) > 0) | (not relu), np.asarray(dzp, F32), F32(0)).astype(np.float64)
        return gd.sum(axis=0), (gd * xhat32(ysel, mean32, invstd32).astype(np.float64)).sum(axis=0)


def grad_constants32(s1, s2, rows):
    """-> (k1, k2, dgamma, dbeta) as float32 from the float64 sums"""
    inv_n = 1.0 / float(rows)
    return f32(s1 * inv_n), f32(s2 * inv_n), f32(s2), f32(s1)


def grad_apply32(y, g32, on, sc, mean32, invstd32, k1, k2):
    """dy = sc * fma(-xh, k2, gk - k1), gk = on ? g : 0"""
    gk = np.where(on, np.asarray(g32, F32), F32(0)).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(sc, F32) * fma32(-xhat32(y, mean32, invstd32), k2, gk - np.asarray(k1, F32))).astype(F32)


def restate(y, gamma, beta, relu, mean32, invstd32, dz=None, pool=0):
    """Everything the kernels derive from (y, saved moments[, dz]) -> dict of float32 arrays: sc, sh, z, on[, zmax, ties, ysel]
    [, g, k1, k2, dgamma, dbeta, dy][, and the pooled reduction's k1p, k2p, dgammap, dbetap].  dz: (rows, c), or (rows / pool, c)
    behind the max pool."""
    y = np.asarray(y, F32)
    r = {}
    r["sc"], r["sh"] = scale_shift32(gamma, beta, mean32, invstd32)
    r["z"], r["on"] = apply32(y, r["sc"], r["sh"], relu)
    if pool > 1:
        r["zmax"], r["ties"], r["ysel"] = pool32(r["z"], y, pool)
    if dz is None:
        return r
    r["g"] = incoming32(r["z"], pool, r["zmax"], r["ties"], dz) if pool > 1 else np.asarray(dz, F32)
    s1, s2 = grad_sums(y, r["g"], r["on"], mean32, invstd32)
    r["k1"], r["k2"], r["dgamma"], r["dbeta"] = grad_constants32(s1, s2, y.shape[0])
    r["dy"] = grad_apply32(y, r["g"], r["on"], r["sc"], mean32, invstd32, r["k1"], r["k2"])
    if pool > 1:
        p1, p2 = grad_sums_pooled(dz, r["zmax"], r["ysel"], relu, mean32, invstd32)
        r["k1p"], r["k2p"], r["dgammap"], r["dbetap"] = grad_constants32(p1, p2, y.shape[0])
    return r


# ----------------------------------------------------------------------------------------------------- 3. tolerance helper
def bound(restated32, ref64, per_channel=False):
    """-> (bound, measured): measured = max |restatement - reference|, bound = max(4 * measured, 1 float32 ulp of max |reference|).
    per_channel (2-D: over the rows of each column; 1-D: each entry by itself): `measured` is taken per channel, the floor
    stays 1 ulp of the whole output's scale.  Non-finite reference entries are left out of both."""
    ref = np.asarray(ref64, np.float64)
    err = np.abs(np.asarray(restated32, np.float64) - ref)
    ok = np.isfinite(ref)
    err = np.where(ok, err, 0.0)
    scale = np.abs(np.where(ok, ref, 0.0)).max() if ref.size else 0.0
    floor = float(ulp32(scale))
    if per_channel:
        measured = err.max(axis=0) if err.ndim == 2 else err
    else:
        measured = float(err.max()) if err.size else 0.0
    return np.maximum(4.0 * measured, floor), measured


def moments_two_pass(col):
    """exact-sum two-pass (mean, biased variance) of one channel, math.fsum"""
    import math
    v = [float(x) for x in np.asarray(col, np.float64)]
    mean = math.fsum(v) / len(v)
    return mean, math.fsum((x - mean) ** 2 for x in v) / len(v)


def cancellation_input(rows=5000, c=8, seed=11):
    """y = 64 + 0.05 * randn rounded to float32: E[y^2] ~ 4096, var ~ 0.0025 -- a one-pass float32 variance is all rounding"""
    return (64.0 + 0.05 * np.random.RandomState(seed).randn(rows, c)).astype(F32)
