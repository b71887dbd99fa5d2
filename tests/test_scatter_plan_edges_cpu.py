"""tests/scatter_ref.py -- the reference, the index tables, the data and the bound of tests/test_scatter_plan_edges_gpu.py -- held
to account without a GPU: against a naive loop, against their own promises (list-length classes, first / last source states,
exactness in any summation order, the bound on general data) and against hand-corrupted plans."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scatter_ref as S  # noqa: E402

ORDERS = 20


def test_scatter_f64_equals_a_naive_loop():
    for b, nsrc, nrows, div, kind in [(1, 1, 1, 1, 0), (2, 5, 7, 3, 1), (3, 11, 9, 3, 2), (2, 4, 13, 1, 0), (1, 300, 5, 3, 1)]:
        idx = S.make_idx(b, nsrc, nrows, div, 3 + nsrc)
        rows, wdata = S.general_data(idx, div, 5, kind, 4 + nsrc)
        w = None if kind == 0 else S.entry_weights(b, idx.shape[1], kind, wdata)
        got, want = S.scatter_f64(idx, rows, w, div, nsrc), S.scatter_naive(idx, rows, w, div, nsrc)
        for g, r in zip(got, want):
            np.testing.assert_allclose(g, r, rtol=1e-15, atol=0)       # the same float64 terms in the same (entry) order
        assert got[2].sum() == idx.size


def test_weights_f32_is_float32_throughout():
    """against the float64 quotient: within 3 roundings; the clamp gives the weight of a zero distance; exact patterns exact"""
    rs = np.random.RandomState(0)
    d = (10.0 ** rs.uniform(-6, 3, (1000, 3))).astype(np.float32)
    w = S.weights_f32(d)
    r = 1.0 / d.astype(np.float64)
    assert w.dtype == np.float32 and np.abs(w / (r / r.sum(1, keepdims=True)) - 1).max() < 4 * S.U * 2
    z = S.weights_f32(np.array([[0.0, 0.5, 2.0], [0.0, 0.0, 1.0]], np.float32))
    assert z[0, 0] == np.float32(1e10) / ((np.float32(1e10) + np.float32(2.0)) + np.float32(0.5)) and z[1, 0] == 0.5 == z[1, 1]
    e = S.weights_f32(np.array([[4.0, 4.0, 2.0], [0.25, np.inf, 0.25], [np.inf, 8.0, np.inf]], np.float32))
    assert np.array_equal(e, np.array([[0.25, 0.25, 0.5], [0.5, 0, 0.5], [0, 1, 0]], np.float32))


def test_index_maker_hits_the_class_edges():
    """make_idx on a table with room: every list length of {0, 1, 2, 3, 4, 5, 7, 8, 9} in EVERY cloud, a hot source, rows of three
    equal indices, tables that differ between clouds, and over four clouds all four (first, last) source states; over the apply
    cases the GPU test uses: every class in every case with at least 11 sources, both states of both ends in the sweep of every c"""
    for div in (1, 3):
        idx = S.make_idx(4, 40, 200 // div, div, 7)
        for t in idx:
            lens, _, share, eq = S.idx_facts(t[None], 40, div)
            assert lens >= set((0,) + S.CLASSES) and share > 0.25 and (div == 1 or eq >= 10), (lens, share, eq)
        assert set(S.idx_facts(idx, 40, div)[1]) == {(False, False), (False, True), (True, False), (True, True)}
        assert len(set(t.tobytes() for t in idx)) == 4
        assert idx.min() >= 0 and idx.max() < 40 and idx.dtype == np.int32
    first, last = {}, {}
    for c, nsrc, b, div, kind in S.apply_cases():
        idx = S.apply_case(c, nsrc, b, div, kind)[0]
        assert idx.shape == (b, S.apply_rows(nsrc, div) * div) and idx.min() >= 0 and idx.max() < nsrc
        lens, ends, share, eq = S.idx_facts(idx, nsrc, div)
        if nsrc >= 11:
            assert lens >= set((0,) + S.CLASSES), (c, nsrc, b, div, lens)
        assert share >= 0.2 and (div == 1 or eq >= 3), (c, nsrc, b, div, share, eq)
        if nsrc >= 3:
            first.setdefault(c, set()).update(e[0] for e in ends)
            last.setdefault(c, set()).update(e[1] for e in ends)
    assert all(first[c] == {True, False} and last[c] == {True, False} for c in S.APPLY_C)


def orders_agree(idx, rows, w32, div, nsrc, seed):
    ref = S.scatter_f64(idx, rows, w32, div, nsrc)[0]
    assert S.is_exact(rows, w32, idx, div, nsrc)
    rs = np.random.RandomState(seed)
    want = S.bits(ref)
    assert np.array_equal(want.view(np.float32).astype(np.float64), ref)          # float32 holds the float64 result
    for k in range(ORDERS):
        assert np.array_equal(S.bits(S.ordered_sums_f32(idx, rows, w32, div, nsrc, rs, fma=False)), want), "order %d" % k
    assert np.array_equal(S.bits(S.ordered_sums_f32(idx, rows, w32, div, nsrc, rs, fma=True)), want)


@pytest.mark.parametrize("c", S.APPLY_C)
def test_exact_data_is_exact_in_any_order_apply_cases(c):
    """every exact_data case of the GPU column sweep: float32 sequential sums without fma in 20 random list orders (and one with
    fma) are bit-equal to each other and to the float64 result"""
    for cc, nsrc, b, div, kind in S.apply_cases():
        if cc == c:
            idx, rows, _, w32 = S.apply_case(cc, nsrc, b, div, kind)
            orders_agree(idx, rows, w32, div, nsrc, c + nsrc)


def test_exact_data_is_exact_in_any_order_build_cases():
    """the same for the single-build and multi-build cases of the GPU test (c = 4)"""
    for case in S.build_cases():
        idx, rows, _, w32 = S.build_case(*case)
        orders_agree(idx, rows, w32, case[3], case[1], case[1])
    for name in S.MULTI_BATCHES:
        for i, (nsrc, nrows, div, kind) in enumerate(S.multi_specs(name)):
            idx, rows, _, w32 = S.multi_case(name, i)
            assert idx.shape == (S.MULTI_B[name], nrows * div)
            orders_agree(idx, rows, w32, div, nsrc, i)


def test_multi_batches_cover_what_they_claim():
    ns = set(n for name in S.MULTI_BATCHES if name.startswith("lds") for n in S.MULTI_BATCHES[name])
    assert ns == {1, 63, 64, 65, 1023, 1024, 1025, 2049, 16384}
    assert max(S.MULTI_BATCHES["global8"]) == 16385 and sorted(S.MULTI_BATCHES["global8"])[:-1] == sorted(S.MULTI_BATCHES["lds8_max"])[:-1]
    assert set(len(v) for v in S.MULTI_BATCHES.values()) == {1, 8}
    for name in ("lds8", "lds8_max", "global8"):
        assert set(k for _, _, _, k in S.multi_specs(name)) == {0, 1, 2}
    words = [S.plan_words(S.MULTI_B["lds8"], r * d, n) for n, r, d, _ in S.multi_specs("lds8")]
    assert any(w % 4 for w in words[:-1]), "no plan of lds8 ends off a 16-byte boundary: the padding between slices goes untested"
    for name in S.MULTI_BATCHES:                        # the largest case stays at a few thousand entries
        assert max(r * d for _, r, d, _ in S.multi_specs(name)) <= 4300


@pytest.mark.parametrize("case", S.GENERAL_CASES, ids=lambda v: "c%d-nsrc%d-b%d-div%d-kind%d" % v)
def test_general_data_bound_holds_for_the_reference(case):
    """float32 sums in 20 random orders, with a rounded product (no fma) and with an exact one (fma), stay inside
    (L + 2) 2^-24 sum_abs of the float64 result on every general-data case of the GPU test; the worst ratio is well inside 1
    (a bound that the reference itself only just met would be no bound to hold a kernel to)"""
    c, nsrc, b, div, kind = case
    idx, rows, _, w32 = S.apply_case(c, nsrc, b, div, kind, exact=False)
    ref, sa, L = S.scatter_f64(idx, rows, w32, div, nsrc)
    bd = S.bound(sa, L)
    assert not S.is_exact(rows, w32, idx, div, nsrc)
    assert S.idx_facts(idx, nsrc, div)[2] >= 0.2                       # the hot source
    assert kind != 2 or (np.float32(1e10) / (np.float32(1e10) + np.float32(1e10))) in w32           # two clamped distances
    rs = np.random.RandomState(c)
    worst = 0.0
    for k in range(ORDERS):
        for fma in (False, True):
            err = np.abs(S.ordered_sums_f32(idx, rows, w32, div, nsrc, rs, fma).astype(np.float64) - ref)
            assert (err <= bd).all(), "order %d fma %d: %.3g of the bound" % (k, fma, (err / np.maximum(bd, 1e-300)).max())
            worst = max(worst, float((err[bd > 0] / bd[bd > 0]).max()))
    assert ((bd == 0) == (L == 0)[..., None]).all()
    print("[scatter_edges] cpu general c=%d nsrc=%d b=%d div=%d kind=%d: worst err/bound %.3g" % (case + (worst,)))
    assert worst < 0.75


def corruptions(cnt, off, eq, ew, idx, nsrc):
    """three plans that are wrong by one entry or one offset"""
    n = np.bincount(idx[0], minlength=nsrc)
    s = int(np.flatnonzero((n[:-1] > 0) & (n[1:] > 0))[0])          # two neighbouring non-empty lists
    moved = [a.copy() for a in (cnt, off, eq, ew)]                  # the last entry of s handed to s + 1: lengths and start move
    moved[0][0, s] -= 1
    moved[0][0, s + 1] += 1
    moved[1][0, s + 1] -= 1
    dup = [a.copy() for a in (cnt, off, eq, ew)]                    # the first entry of s + 1 overwritten by the last of s
    p = int(off[0, s + 1])
    dup[2][0, p], dup[3][0, p] = eq[0, p - 1], ew[0, p - 1]
    shifted = [a.copy() for a in (cnt, off, eq, ew)]                # one offset off by one, everything else as built
    shifted[1][0, s + 1] += 1
    return {"moved": moved, "duplicated": dup, "offset": shifted}


@pytest.mark.parametrize("div,kind", S.MODES)
def test_check_plan_accepts_valid_plans_and_rejects_corrupted_ones(div, kind):
    b, nsrc, nrows = 2, 37, 120
    idx = S.make_idx(b, nsrc, nrows, div, 11)
    rows, wdata = S.general_data(idx, div, 4, kind, 12)
    w32 = S.entry_weights(b, idx.shape[1], kind, wdata)
    for rs in (None, np.random.RandomState(5)):                     # list order is free
        plan = S.build_plan_host(idx, w32, div, nsrc, rs)
        S.check_plan(*plan, idx, w32, div, nsrc)
        again = S.decode_plan(S.encode_plan(*plan), b, idx.shape[1], nsrc)
        assert all(np.array_equal(S.bits(a) if a.dtype == np.float32 else a, S.bits(p) if p.dtype == np.float32 else p)
                   for a, p in zip(again, plan))
    for name, bad in corruptions(*plan, idx, nsrc).items():
        assert any(not np.array_equal(S.bits(a), S.bits(p)) for a, p in zip(bad[1:], plan[1:])), name
        with pytest.raises(AssertionError):
            S.check_plan(*bad, idx, w32, div, nsrc)
    one_ulp = [a.copy() for a in plan]                              # membership is exact: a weight one ulp off is no member
    one_ulp[3] = (S.bits(plan[3]) + np.uint32(1)).view(np.float32)
    with pytest.raises(AssertionError):
        S.check_plan(*one_ulp, idx, w32, div, nsrc)
    with pytest.raises(AssertionError):
        S.decode_plan(S.encode_plan(*plan)[:-4], b, idx.shape[1], nsrc)


def block_scan(cnt, threads, per):
    """the build's exclusive scan as its kernels arrange it: thread t owns the counters [t per, (t + 1) per) -> offsets, with the
    value a poisoned plan holds (-1 here) wherever no thread writes"""
    m = cnt.size
    off = np.full(m, -1, np.int64)
    run = 0
    for t in range(threads):
        lo, hi = min(t * per, m), min(t * per + per, m)
        for i in range(lo, hi):
            off[i] = run
            run += cnt[i]
    return off


@pytest.mark.parametrize("nsrc", S.BUILD_NSRC)
def test_check_plan_catches_a_scan_that_drops_its_tail(nsrc):
    """the 256-thread scan emulated on the host with per = ceil(m / 256) (as built) and with per = m / 256 (rounded down: the
    counters past 256 per are never visited): check_plan accepts the first at every source count of the single-build sweep and
    rejects the second at every one that is no multiple of 256"""
    idx, _, _, w32 = S.build_case(2, nsrc, 257, 3, 1)
    cnt, off, eq, ew = S.build_plan_host(idx, w32, 3, nsrc)
    good = np.stack([block_scan(c, 256, (nsrc + 255) // 256) for c in cnt]).astype(np.int32)
    assert np.array_equal(good, off)
    bad = np.stack([block_scan(c, 256, nsrc // 256) for c in cnt]).astype(np.int32)
    if nsrc % 256 == 0:
        S.check_plan(cnt, bad, eq, ew, idx, w32, 3, nsrc)
    else:
        with pytest.raises(AssertionError):
            S.check_plan(cnt, bad, eq, ew, idx, w32, 3, nsrc)
