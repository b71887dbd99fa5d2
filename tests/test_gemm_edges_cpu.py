"""The host model of the dense-layer GEMM family (tests/gemm_ref.py) checked on its own, and the coverage claims of
tests/test_gemm_edges_gpu.py proved without a GPU: every branch of the dispatch mirrors has a case, every threshold has a case on
each side, and every case is exact (all products, partial sums and statistics terms are integers below 2^24)."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as B  # noqa: E402
import gemm_ref as R  # noqa: E402

CASES = R.all_cases()


def _clip(c):
    """rows of the case for a host-side reference: the row count itself up to 300, then 256 + rows % 32 (the references do not
    depend on the dispatch; pooling needs rows % pool kept)"""
    if c.get("pool", 0) > 32:
        return 192
    return c["rows"] if c["rows"] <= 300 else 256 + c["rows"] % 32


def test_case_tables_are_exact_below_2_to_24():
    bad = [(c["kind"], c["rows"], b) for c in CASES for b in c["bounds"] if not R.exact_bound_ok(*b)]
    assert not bad, bad[:5]
    # the check itself refuses what is not exact
    assert R.exact_bound_ok(256, 2, 2) and not R.exact_bound_ok(256, 2, 2, stats="y") and R.exact_bound_ok(255, 2, 2, stats="y")
    assert R.exact_bound_ok(1023, 1, 1, stats="y") and not R.exact_bound_ok(1024, 1, 1, stats="y")
    assert not R.exact_bound_ok(1 << 22, 2, 2) and not R.exact_bound_ok(10, 2, 2, start=1 << 24)
    assert R.stats_mag(255) == (2, 2) and R.stats_mag(256) == (2, 1) and R.stats_mag(768) == (1, 1)


def test_operands_stay_inside_the_magnitudes_the_bounds_assume():
    """what make_operands draws (at clipped rows) is integer valued and bounded by the (amax, bmax) of the case's bounds"""
    for c in CASES[::3]:
        o = R.make_operands(c, _clip(c))
        k, amax, bmax, start, _ = c["bounds"][0]
        if c["kind"] in ("linear", "bn_stats", "xf"):
            a, b = o["a"], o["w"]
        elif c["kind"] in ("dgrad", "dgrad_gx", "fused"):
            a, b = o["dy"], o["w"]
        else:
            a, b = o["a"], o["dy"]
        assert np.abs(R.to_int(a)).max() <= amax and np.abs(R.to_int(b)).max() <= bmax, (c["kind"], c["rows"])
        if c["kind"] == "fused" and len(c["bounds"]) > 1:
            _, a2, b2, _, _ = c["bounds"][1]
            assert np.abs(R.to_int(o["a"])).max() <= a2 and np.abs(o["dy"]).max() <= b2


def test_every_branch_of_the_dispatch_mirrors_has_a_case():
    hit = collections.Counter(c["branch"] for c in CASES)
    universe = R.branch_universe()
    assert not universe - set(hit), sorted(universe - set(hit))
    assert not set(hit) - universe, sorted(set(hit) - universe)


def test_every_threshold_has_a_case_on_each_side():
    sides = collections.defaultdict(set)
    for c in CASES:
        for name, outcome in c["trail"]:
            sides[name].add(outcome)
    assert len(sides) >= 29
    one_sided = sorted(n for n, s in sides.items() if s != {True, False})
    assert not one_sided, one_sided


def test_threshold_row_counts_of_the_mirrors():
    """the row counts at which the shipped build changes tiles, worked out by hand from the conditions in the source"""
    f = lambda *a, **k: R.linear_impl(*a, **k)[0]
    assert f(2048, 36, 32) == "splitk<1,1,2>/vec" and f(2049, 36, 32) == "lds<4,1,1>/vec"
    assert f(2048, 36, 32, pool=16).startswith("lds<4,1,1>")            # pool 16 has no split-K form
    assert f(32768, 36, 64) == "lds<1,2,1,2>/cout%64/vec" and f(32769, 36, 64) == "lds<4,1,2>/vec"
    assert f(2080, 36, 64, pool=32) == "lds<4,1,2>/vec"
    assert f(8160, 128, 128) == "lds<1,2,1,2>/cout%128/vec" and f(8161, 128, 128) == "lds<1,4,1>/vec"
    assert f(8160, 36, 128) == "lds<1,4,1>/vec"                          # cin < 128
    assert f(4064, 128, 256) == "lds<1,2,1,2>/cout%128/vec" and f(4065, 128, 256) == "lds<1,4,1>/vec"
    assert f(8128, 128, 512) == "lds<1,4,1>/vec" and f(8129, 128, 512) == "lds<2,2,2>/vec"
    assert f(16256, 128, 512) == "lds<2,2,2>/vec" and f(16257, 128, 512) == "lds<4,1,4>/vec"
    assert f(16257, 130, 512) == "lds<2,2,2>/scalar" and f(16257, 128, 512, aligned=False) == "lds<2,2,2>/scalar"
    assert f(32704, 128, 128) == "lds<1,4,1>/vec" and f(32705, 128, 128) == "lds<2,2,2>/vec"
    assert f(65536, 64, 128, stats=True) == "fwd_narrow<64,128>" and f(65535, 64, 128, stats=True) == "lds<2,2,2>/vec"
    assert f(65536, 64, 128) == "lds<2,2,2>/vec"                         # without the statistics epilogue
    g = lambda *a, **k: R.linear_dgrad_impl(*a, **k)[0]
    assert g(16320, 129, 36) == "dgrad<1,4,1>/vec/b4" and g(16321, 256, 36) == "dgrad<2,2,2>/vec/b4"
    assert g(32768, 128, 9) == "smallk<9>/reg" and g(32769, 128, 9) == "smallk<9>/reg/capped"
    assert g(257, 128, 9, dx_aligned=False) == "smallk<9>/lds" and g(257, 12, 9) == "smallk<9>/lds"
    assert g(65536, 128, 128, gx=1) == "dgrad_wide<128>/gx1" and g(65504, 128, 128, gx=1) == "dgrad<2,2,2>/gx1/b4"
    assert g(64, 33, 16, gx=1) == "EUNSUP" and g(64, 33, 516, gx=1) == "EUNSUP" and g(64, 33, 18, gx=1) == "EUNSUP"
    p = R.wgrad_plan(65537, 128, 128)
    assert p["wide8"] and p["gy"] == 2 and p["chunk"] == 72 and p["nchunks"] == 911 and p["last_rows"] == 17   # 1024 waves
    p = R.wgrad_plan(129, 33, 33)
    assert (p["tm"], p["tn"], p["chunk"], p["nchunks"], p["last_rows"], p["last_live"]) == (2, 2, 32, 5, 1, 1)
    for live in (1, 2, 3):
        q = R.wgrad_plan(R.wgrad_rows_with(67, 131, live), 67, 131)
        assert q["last_rows"] == 1 and q["last_live"] == live


def test_integer_references_agree_with_float64():
    """int64 y / dx / dw and both pairs of column sums against float64 matmuls of the same operands, on every case"""
    for c in CASES:
        o = R.make_operands(c, _clip(c))
        kind = c["kind"]
        if kind in ("linear", "bn_stats", "xf"):
            acc, y = R.ref_forward(o["a"], o["w"], o["bias"], c.get("relu", 0), c.get("pool", 0))
            f = o["a"].astype(np.float64) @ o["w"].astype(np.float64)
            assert np.array_equal(acc, f)
            g = f + (o["bias"].astype(np.float64) if o["bias"] is not None else 0.0)
            g = np.maximum(g, 0.0) if c.get("relu") else g
            g = g.reshape(-1, c["pool"], g.shape[1]).max(axis=1) if c.get("pool", 0) > 1 else g
            assert np.array_equal(y, g)
            s1, s2 = R.ref_column_stats(acc)
            assert np.array_equal(s1, f.sum(axis=0)) and np.array_equal(s2, (f * f).sum(axis=0))
        if kind in ("dgrad", "dgrad_gx", "fused"):
            dx = R.ref_dgrad(o["dy"], o["w"])
            f = o["dy"].astype(np.float64) @ o["w"].astype(np.float64).T
            assert np.array_equal(dx, f)
            if "below" in o:
                yb, gamma, beta, mean, invstd = (np.asarray(a, np.float64) for a in o["below"])
                s1, s2 = R.ref_grad_stats(dx, o["below"], c["relu_below"])
                sc = gamma * invstd
                on = (yb * sc + (beta - mean * sc) > 0) if c["relu_below"] else np.ones(yb.shape, bool)
                gd = np.where(on, f, 0.0)
                assert np.array_equal(s1, gd.sum(axis=0)) and np.array_equal(s2, (gd * ((yb - mean) * invstd)).sum(axis=0))
        if kind in ("wgrad", "wgrad_xf", "wgrad_gx", "fused"):
            dw = R.ref_wgrad(o["a"], o["dy"], o["dw0"])
            f = o["a"].astype(np.float64).T @ o["dy"].astype(np.float64) + (o["dw0"] if o["dw0"] is not None else 0.0)
            assert np.array_equal(dw, f)


@pytest.mark.parametrize("relu", [0, 1])
def test_element_restatements_equal_bn_ref(relu):
    """load_transform32 / grad_element32 / grad_element_pooled32 against bn_ref's apply32 / grad_apply32 / pool32 / incoming32 on
    shared general (non-integer) inputs, bit for bit"""
    rs = np.random.RandomState(5 + relu)
    rows, c = 192, 24
    y = (rs.randn(rows, c) * (1 + rs.rand(c)) + rs.randn(c)).astype(np.float32)
    gamma, beta = (1 + 0.3 * rs.randn(c)).astype(np.float32), (0.2 * rs.randn(c)).astype(np.float32)
    mean, invstd = rs.randn(c).astype(np.float32), (0.5 + rs.rand(c)).astype(np.float32)
    sc, sh = B.scale_shift32(gamma, beta, mean, invstd)
    z, on = B.apply32(y, sc, sh, relu)
    assert np.array_equal(R.load_transform32(y, sc, sh, relu), z)
    k1, k2 = (0.05 * rs.randn(c)).astype(np.float32), (0.05 * rs.randn(c)).astype(np.float32)
    coef = np.stack([sc, sh, mean, invstd, k1, k2])
    dz = rs.randn(rows, c).astype(np.float32)
    assert np.array_equal(R.grad_element32(y, dz, coef, relu), B.grad_apply32(y, dz, on, sc, mean, invstd, k1, k2))
    y[32:40] = y[40:48]        # exact ties inside a group
    z, on = B.apply32(y, sc, sh, relu)
    zmax, ties, _ = B.pool32(z, y, 32)
    m2, n2 = R.pooled_max_ties32(y, coef, relu)
    assert np.array_equal(zmax, m2) and np.array_equal(ties, n2) and ties.max() >= 2
    dzp = rs.randn(rows // 32, c).astype(np.float32)
    g = B.incoming32(z, 32, zmax, ties, dzp)
    assert np.array_equal(R.grad_element_pooled32(y, dzp, zmax, ties, coef, relu), B.grad_apply32(y, g, on, sc, mean, invstd, k1, k2))


def test_gamma_bound_holds_for_a_float32_dot_product_in_any_order():
    rs = np.random.RandomState(3)
    a, b = rs.randn(7, 300).astype(np.float32), rs.randn(300, 5).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    bound = R.gamma_bound(300, np.abs(a), np.abs(b))
    for order in (np.arange(300), np.arange(300)[::-1], rs.permutation(300)):
        acc = np.zeros((7, 5), np.float32)
        for k in order:
            acc = B.fma32(a[:, k:k + 1], b[k:k + 1, :], acc)
        assert np.all(np.abs(acc.astype(np.float64) - ref) <= bound)
    assert bound.max() < 1e-3 * np.abs(ref).max() + 1e-2
