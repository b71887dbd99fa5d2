"""Host model of the dense-layer GEMM family (csrc/pn2_linear.hip, pn2_fwd_narrow.h, pn2_dgrad_wide.h, pn2_bwd_fused.hip), numpy only.

Five parts:
  1. integer operand makers: x, w, dy, bias and the per-channel vectors are small integers (the batch-norm constants +-1, 2 and
     small integers), chosen so that the A operand a kernel FORMS -- x itself, relu(fma(x, sc, sh)), pn2_bn_grad_element(...) or
     pn2_bn_grad_element_pooled(...) -- is itself a small integer.  The bound of each form is in AMAX;
  2. the float32 restatement of the load transform and of the two gradient-element functions, operation by operation
     (fma32 / f32 of bn_ref.py);
  3. `exact_bound_ok`: with |A| <= amax, |B| <= bmax and a contraction of k terms every product and every partial sum of every
     summation order is an integer of magnitude <= k * amax * bmax (+ the start value); below 2^24 it is a float32 and the result
     does not depend on the order, the split or the atomics.  The statistics epilogues add 16 terms of y and y * y per lane;
  4. int64 references of y (bias / ReLU / max over groups of rows), dx, dw (from a start value) and both pairs of column sums;
  5. mirrors of the dispatch functions: shape -> (name of the branch, the decisions taken on the way), written from the
     conditions in the source for the shipped build (g_lin_cfg = 0, narrow = 1, wide8 = 1, minimum chunk 32, stream rows 65536),
     and the case tables of tests/test_gemm_edges_*.py built on them.
`gamma_bound` is the bound for general (non-integer) data.
"""
import numpy as np

from bn_ref import F32, f32, fma32

EXACT = 1 << 24
STREAM_MIN_ROWS = 65536
WGRAD_MIN_CHUNK = 32
BN_HEAD, BN_SLOTS = 48, 64


# ------------------------------------------------------------------------------------------ 2. float32 element restatements
def load_transform32(x, sc, sh, relu):
    """a = relu?(fma(x, sc[k], sh[k])): store_tile's XF branch, linear_wgrad_kernel's XF operand"""
    t = fma32(x, sc, sh)
    return np.maximum(t, F32(0)) if relu else t


def grad_element32(y, g_in, coef, relu):
    """pn2_bn_grad_element; coef (6, c) = sc, sh, mu, is, k1, k2"""
    sc, sh, mu, is_, k1, k2 = (np.asarray(coef[j], F32) for j in range(6))
    y = np.asarray(y, F32)
    lin = fma32(y, sc, sh)
    on = (lin > 0) if relu else np.ones(lin.shape, bool)
    gk = np.where(on, np.asarray(g_in, F32), F32(0)).astype(F32)
    xh = ((y - mu).astype(F32) * is_).astype(F32)
    return (sc * fma32(-xh, k2, (gk - k1).astype(F32))).astype(F32)


def grad_element_pooled32(y, d, m, n, coef, relu, pool=32):
    """pn2_bn_grad_element_pooled; d, m, n (rows / pool, c): pooled gradient, pooled maximum, rows attaining it"""
    sc, sh, mu, is_, k1, k2 = (np.asarray(coef[j], F32) for j in range(6))
    y = np.asarray(y, F32)
    rep = lambda a: np.repeat(np.asarray(a, F32), pool, axis=0)
    lin = fma32(y, sc, sh)
    on = (lin > 0) if relu else np.ones(lin.shape, bool)
    t = np.where(on, lin, F32(0)).astype(F32)
    g = np.where(t == rep(m), (rep(d) / rep(n)).astype(F32), F32(0)).astype(F32)
    gk = np.where(on, g, F32(0)).astype(F32)
    xh = ((y - mu).astype(F32) * is_).astype(F32)
    return (sc * fma32(-xh, k2, (gk - k1).astype(F32))).astype(F32)


def pooled_max_ties32(y, coef, relu, pool=32):
    """what pn2_bn_relu_forward leaves beside the pooled output: (zmax, ties) of t = relu?(fma(y, sc, sh)) over groups of rows"""
    lin = fma32(y, coef[0], coef[1])
    t = (np.maximum(lin, F32(0)) if relu else lin).reshape(-1, pool, lin.shape[1])
    m = t.max(axis=1)
    return m.astype(F32), (t == m[:, None, :]).sum(axis=1).astype(F32)


# ------------------------------------------------------------------------------------------------- 1. integer operand makers
# |operand| <= AMAX[form] by construction (asserted by the makers)
AMAX = {"plain": 2, "unit": 1, "xf": 4, "gx": 7, "gxp": 37}


def ints(rs, shape, mag):
    return rs.randint(-mag, mag + 1, size=shape).astype(F32)


def make_xf(rs, rows, cin):
    """x in [-2, 2], scale +-1, shift 1 or 2 (> 0: an unmasked padded element is non-zero) -> (x, sc, sh); |a| <= 4"""
    x = ints(rs, (rows, cin), 2)
    sc = rs.choice([-1.0, 1.0], size=cin).astype(F32)
    sh = rs.choice([1.0, 2.0], size=cin).astype(F32)
    return x, sc, sh


def make_coef(rs, c):
    """coef (6, c): sc +-1, sh in {-1, 0, 1}, mean in {0, 1}, invstd in {1, 2}, k1 and k2 in {-1, 0, 1}"""
    return np.stack([rs.choice([-1.0, 1.0], size=c), rs.randint(-1, 2, c), rs.randint(0, 2, c), rs.choice([1.0, 2.0], size=c),
                     rs.randint(-1, 2, c), rs.randint(-1, 2, c)]).astype(F32)


def make_gx(rs, rows, c, relu):
    """y in [-1, 1], dz in [-2, 2] -> (y, dz, coef, dy); |dy| <= |xh| * |k2| + |g| + |k1| = 4 + 2 + 1"""
    coef = make_coef(rs, c)
    y, dz = ints(rs, (rows, c), 1), ints(rs, (rows, c), 2)
    dy = grad_element32(y, dz, coef, relu)
    assert np.abs(dy).max() <= AMAX["gx"] and np.array_equal(dy, np.rint(dy))
    return y, dz, coef, dy


def make_gx_pooled(rs, rows, c, relu, pool=32):
    """y = sc * u with u <= top on a power-of-two number of rows of each (group, channel): the tie counts are powers of two (32
    where the ReLU zeroes the whole group); the pooled gradient is a multiple of 32 -> (y, dzp, zmax, ties, coef, dy); |dy| <= 37"""
    g = rows // pool
    coef = make_coef(rs, c)
    top = rs.randint(-1, 2, size=(g, 1, c))
    u = top - rs.randint(1, 3, size=(g, pool, c))
    ntie = 1 << rs.randint(0, 6, size=(g, 1, c))
    order = rs.rand(g, pool, c).argsort(axis=1)      # a random set of `ntie` rows per (group, channel)
    u = np.where(order < ntie, top, u)
    y = (u * coef[0]).reshape(rows, c).astype(F32)   # fma(y, sc, sh) = u + sh
    zmax, ties = pooled_max_ties32(y, coef, relu, pool)
    assert np.all((ties.astype(np.int64) & (ties.astype(np.int64) - 1)) == 0)
    dzp = (32 * rs.randint(-1, 2, size=(g, c))).astype(F32)
    dy = grad_element_pooled32(y, dzp, zmax, ties, coef, relu, pool)
    assert np.abs(dy).max() <= AMAX["gxp"] and np.array_equal(dy, np.rint(dy))
    return y, dzp, zmax, ties, coef, dy


def make_below(rs, rows, c):
    """batch norm of the layer below (Pn2BnGradEpilogue): y in [-2, 2], gamma +-1, beta in {-1, 0, 1}, mean in {0, 1}, invstd
    in {1, 2}: xhat is an integer of magnitude <= XHMAX"""
    y = ints(rs, (rows, c), 2)
    return (y, rs.choice([-1.0, 1.0], size=c).astype(F32), rs.randint(-1, 2, c).astype(F32), rs.randint(0, 2, c).astype(F32),
            rs.choice([1.0, 2.0], size=c).astype(F32))


XHMAX = 6


# ------------------------------------------------------------------------------------------------------- 3. exactness check
def exact_bound_ok(k, amax, bmax, start=0, stats=None):
    """every product, every partial sum (any order, any split) and every statistics term of a case is an integer below 2^24.
    stats: None, "y" (16 terms of y and of y * y per lane) or "g" (16 terms of g and of g * xhat, |xhat| <= XHMAX)"""
    acc = k * amax * bmax + start
    ok = amax * bmax < EXACT and acc < EXACT
    if stats == "y":
        ok = ok and 16 * acc < EXACT and 16 * acc * acc < EXACT
    elif stats == "g":
        ok = ok and 16 * acc * XHMAX < EXACT
    return bool(ok)


def stats_mag(k):
    """largest operand magnitudes (a, b) of a plain statistics case of contraction k: [-2, 2] up to k = 255, then {-1, 0, 1}"""
    for a, b in ((2, 2), (2, 1), (1, 1)):
        if exact_bound_ok(k, a, b, stats="y"):
            return a, b
    raise ValueError("no exact magnitudes for k = %d" % k)


# ------------------------------------------------------------------------------------------------------ 4. int64 references
def to_int(a):
    a = np.asarray(a)
    r = np.rint(a).astype(np.int64)
    assert np.array_equal(r, a), "operand is not integer valued"
    return r


def int_mm(a, b):
    return to_int(a) @ to_int(b)


def ref_forward(a, w, bias=None, relu=0, pool=0, mm=int_mm):
    """y = a . w [+ bias] [ReLU] [max over groups of `pool` rows] -> (y before the epilogue, output)"""
    acc = mm(a, w)
    y = acc + (to_int(bias) if bias is not None else 0)
    if relu:
        y = np.maximum(y, 0)
    if pool > 1:
        y = y.reshape(-1, pool, y.shape[1]).max(axis=1)
    return acc, y


def ref_column_stats(acc):
    """column sums of y and y * y (push_column_stats)"""
    return acc.sum(axis=0), (acc * acc).sum(axis=0)


def ref_dgrad(dy, w, mm=int_mm):
    """dx = dy . w^T, w (n_in, n_out)"""
    return mm(dy, np.ascontiguousarray(np.asarray(w).T))


def ref_wgrad(x, dy, dw0=None, mm=int_mm):
    """dw = dw0 + x^T . dy"""
    r = mm(np.ascontiguousarray(np.asarray(x).T), dy)
    return r + (to_int(dw0) if dw0 is not None else 0)


def ref_grad_stats(dx, below, relu):
    """column sums of g = dx * [mask] and of g * xhat for the layer below (push_column_grad_stats)"""
    y, gamma, beta, mean, invstd = below
    sc = (gamma * invstd).astype(F32)
    on = (fma32(y, sc, fma32(-mean, sc, beta)) > 0) if relu else np.ones(y.shape, bool)
    g = np.where(on, dx, 0)
    xh = to_int(((y - mean).astype(F32) * invstd).astype(F32))
    assert np.abs(xh).max() <= XHMAX
    return g.sum(axis=0), (g * xh).sum(axis=0)


def gamma_k(k):
    """k u / (1 - k u), u = 2^-24: the relative error bound of a float32 sum of k terms formed in any order"""
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def gamma_bound(k, absA, absB):
    """|fl(A . B) - A . B| <= gamma_k * (|A| . |B|) elementwise for every summation order; k = contraction length + epilogue
    operations, u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 3.5)"""
    return gamma_k(k) * (np.asarray(absA, np.float64) @ np.asarray(absB, np.float64))


# ------------------------------------------------------------------------------------------------------ 5. dispatch mirrors
class Trail(list):
    """the decisions a mirror evaluated on the way: (name, outcome)"""
    def d(self, name, v):
        self.append((name, bool(v)))
        return bool(v)


def fwd_narrow_fits(rows, cin, cout, aligned=True):
    if cin not in (32, 64) and not (cin == 128 and cout == 128):
        return False
    if cout not in (32, 64, 128):
        return False
    if rows % 32 != 0 or rows < STREAM_MIN_ROWS:
        return False
    return bool(aligned)


def dgrad_wide_fits(rows, n_in, n_out, gx, pool=0, aligned=True):
    if not gx or n_out != 128 or n_in not in (64, 128):
        return False
    if pool not in (0, 32):
        return False
    if rows % 32 != 0 or rows < STREAM_MIN_ROWS:
        return False
    return bool(aligned)


def linear_impl(rows, cin, cout, pool=0, aligned=True, stats=False, bias=False, relu=False):
    """-> (branch, trail) of linear_impl; aligned: x on a 16-byte boundary"""
    t = Trail()
    vec = cin % 4 == 0 and aligned
    tag = "/vec" if vec else "/scalar"
    if t.d("fwd.narrow", stats and not bias and not relu and pool <= 1 and fwd_narrow_fits(rows, cin, cout, aligned)):
        return "fwd_narrow<%d,%d>" % (cin, cout), t
    if t.d("fwd.rows<=2048", rows <= 2048 and (pool <= 1 or pool == 32)):
        return "splitk<1,1,2>" + tag, t
    if t.d("fwd.cout%128", cout % 128 == 0):
        cb = cout // 128
        if t.d("fwd.128-row tile", ((rows + 127) // 128) * cb >= 512 and vec and cb > 1):
            return "lds<4,1,4>/vec", t
        if t.d("fwd.64-row tile", ((rows + 63) // 64) * cb >= 512):
            return "lds<2,2,2>" + tag, t
        if t.d("fwd.32-row tile", ((rows + 31) // 32) * cb >= 256 or cin < 128):
            return "lds<1,4,1>" + tag, t
        return "lds<1,2,1,2>/cout%128" + tag, t
    if t.d("fwd.cout%64", cout % 64 == 0):
        if t.d("fwd.cout%64 few rows", pool <= 1 and rows <= 32768):
            return "lds<1,2,1,2>/cout%64" + tag, t
        return "lds<4,1,2>" + tag, t
    return "lds<4,1,1>" + tag, t


def linear_bn_stats_xf_impl(rows, cin, cout):
    """-> (branch, trail) of linear_bn_stats_xf_impl; "EUNSUP" where it refuses"""
    t = Trail()
    if t.d("xf.unsupported", cout % 32 != 0 or cin % 4 != 0 or rows <= 2048):
        return "EUNSUP", t
    if t.d("xf.narrow", fwd_narrow_fits(rows, cin, cout)):
        return "fwd_narrow<%d,%d>/xf" % (cin, cout), t
    if t.d("xf.cout%128", cout % 128 == 0):
        if t.d("xf.64-row tile", ((rows + 63) // 64) * (cout // 128) >= 512):
            return "xf<2,2,2>", t
        return "xf<1,4,1>", t
    if t.d("xf.cout%64", cout % 64 == 0):
        return "xf<4,1,2>", t
    return "xf<4,1,1>", t


def dgrad_smallk(rows, n_in, aligned=True):
    """launch_dgrad_smallk -> (variant, grid capped)"""
    groups = (n_in + 3) // 4
    if n_in % 4 == 0 and groups <= 256 and 256 % groups == 0 and aligned:
        rpb = 256 // groups
        return "reg", (rows + rpb - 1) // rpb > 256 * 16
    return "lds", (rows * groups + 255) // 256 > 256 * 32


def linear_dgrad_impl(rows, n_in, n_out, gx=0, pool=0, aligned=True, dx_aligned=True):
    """-> (branch, trail) of linear_dgrad_impl (cin = n_in, cout = n_out); gx: dy formed on load; aligned: dy on a 16-byte
    boundary; "EUNSUP" where the on-load form is refused"""
    t = Trail()
    if gx and t.d("dgrad.gx unsupported", n_out % 4 != 0 or n_out <= 16 or n_out > 512):
        return "EUNSUP", t
    if t.d("dgrad.small k", n_out <= 16 and n_in * n_out * 4 <= 48 * 1024):
        variant, capped = dgrad_smallk(rows, n_in, dx_aligned)
        t.d("dgrad.small k registers", variant == "reg")
        t.d("dgrad.small k grid cap/" + variant, capped)
        return "smallk<%d>/%s%s" % (n_out, variant, "/capped" if capped else ""), t
    if t.d("dgrad.wide", dgrad_wide_fits(rows, n_in, n_out, gx, pool)):
        return "dgrad_wide<%d>/gx%d" % (n_in, 2 if pool else 1), t
    a = "/gx%d" % (2 if pool else 1) if gx else ("/vec" if n_out % 4 == 0 and aligned else "/scalar")
    a += "/b4" if n_out % 4 == 0 else "/b1"   # transposed B: one 16-byte load or four scalar loads
    if t.d("dgrad.n_in<=32", n_in <= 32):
        return "dgrad<4,1,1>" + a, t
    if t.d("dgrad.n_in<=64", n_in <= 64):
        return "dgrad<4,1,2>" + a, t
    if t.d("dgrad.n_in<=96", n_in <= 96):
        return "dgrad<4,1,1>x3" + a, t
    if t.d("dgrad.64-row tile", ((rows + 63) // 64) * ((n_in + 127) // 128) >= 512):
        return "dgrad<2,2,2>" + a, t
    return "dgrad<1,4,1>" + a, t


def wgrad_plan(rows, cin, cout):
    """the split of linear_wgrad_impl -> dict(tm, tn, gy, gz, wide8, chunk, nchunks, nwg, last_rows, last_live)"""
    tm = 2 if cin > 32 else 1
    tn = 4 if cout > 64 else (2 if cout > 32 else 1)
    gy, gz = (cin + 32 * tm - 1) // (32 * tm), (cout + 32 * tn - 1) // (32 * tn)
    wide8 = tm == 2 and tn == 4 and rows >= STREAM_MIN_ROWS
    waves = max((2048 if wide8 else 1024) // (gy * gz), 16)
    chunk = max(((rows + waves - 1) // waves + 7) & ~7, WGRAD_MIN_CHUNK)
    nchunks = (rows + chunk - 1) // chunk
    nwv = 8 if wide8 else 4
    return dict(tm=tm, tn=tn, gy=gy, gz=gz, wide8=wide8, chunk=chunk, nchunks=nchunks, nwg=(nchunks + nwv - 1) // nwv,
                last_rows=rows - (nchunks - 1) * chunk, last_live=(nchunks - 1) % nwv + 1)


def linear_wgrad_impl(rows, cin, cout, xf=False, gx=0):
    """-> (branch, trail) of linear_wgrad_impl"""
    t = Trail()
    p = wgrad_plan(rows, cin, cout)
    t.d("wgrad.cin>32", cin > 32)
    t.d("wgrad.cout>64", cout > 64)
    if cout <= 64:
        t.d("wgrad.cout>32", cout > 32)
    if p["tm"] == 2 and p["tn"] == 4:
        t.d("wgrad.eight waves", p["wide8"])
    t.d("wgrad.ragged last chunk", p["last_rows"] < p["chunk"])
    return "wgrad<%d,%d>%s%s%s" % (p["tm"], p["tn"], "/8" if p["wide8"] else "/4", "/xf" if xf else "", "/gx%d" % gx if gx else ""), t


def wgrad_rows_with(cin, cout, last_live, last_rows=1, lo=1, hi=20000):
    """smallest row count in [lo, hi) whose last chunk holds `last_rows` rows and whose last workgroup holds `last_live` chunks"""
    for rows in range(lo, hi):
        p = wgrad_plan(rows, cin, cout)
        if p["last_rows"] == last_rows and p["last_live"] == last_live and p["nchunks"] > 1:
            return rows
    raise ValueError("no such row count")


def linear_bwd_fused(rows, cin, cout, pool=0):
    """-> (branch, trail) of pn2_linear_bwd_fused"""
    t = Trail()
    if t.d("fused.unsupported", cin not in (32, 64) or cout not in (32, 64) or rows % 32 != 0):
        return "EUNSUP", t
    return "bwd_narrow<%d,%d>/gx%d" % (cin // 32, cout // 32, 2 if pool else 1), t


# -------------------------------------------------------------------------------------------------------------- case tables
# A case is a dict; `branch` / `trail` come from the mirror, `bounds` = the (k, amax, bmax, start, stats) of each GEMM of the
# case for exact_bound_ok, `amax` / `bmax` the operand magnitudes the test draws.
def _case(kind, mirror, k, amax, bmax, start=0, stats=None, more=(), **kw):
    branch, trail = mirror
    return dict(kind=kind, branch=branch, trail=trail, bounds=[(k, amax, bmax, start, stats)] + list(more), amax=amax, bmax=bmax,
                **kw)


def forward_cases():
    """pn2_linear (bias / ReLU / pool) and, where there is no pool, pn2_linear_bn_stats[_fin] at the same shape"""
    shapes = []
    for rows in (1, 31, 32, 33, 2048):   # split-K <1,1,2>
        for cin in (1, 3, 4, 31, 32, 33, 36, 67):
            for cout in (32, 96):
                for pool in (0, 32):
                    if pool and rows % pool:
                        continue
                    for xoff in (0, 1):
                        shapes.append((rows, cin, cout, pool, xoff))
    shapes += [(r, 36, c, 0, 0) for r in (2049, 32768) for c in (64, 192)]            # <1,2,1,2> via cout % 64
    shapes += [(32769, 36, 64, 0, 0)] + [(2080, 36, 64, p, 0) for p in (16, 32)]  # <4,1,2>
    shapes += [(r, 33, c, 0, 0) for r in (2049, 2175) for c in (32, 96, 160)]         # <4,1,1>
    shapes += [(2112, 36, 96, p, 0) for p in (16, 32, 96)] + [(2112, 36, 64, 64, 1)]   # (2080 % 64 != 0: refused, see the contracts)
    shapes += [(2049, 33, 64, 0, 0), (2049, 36, 64, 0, 1)]                              # the same tiles with scalar A loads
    shapes += [(32, 36, 32, 16, 0), (2048, 36, 64, 16, 1)]                              # pool 16 has no split-K form
    shapes += [(2049, 36, 128, 0, 0)]                                                  # <1,4,1> through cin < 128
    shapes += [(r, k, 128, 0, 0) for r in (2049, 8160, 8161) for k in (128, 131, 132)]  # <1,2,1,2> via cout % 128 | <1,4,1>
    shapes += [(r, 128, 256, 0, 0) for r in (4064, 4065)]
    shapes += [(r, 128, 512, 0, 0) for r in (8128, 8129, 16256, 16257)]               # <1,4,1> | <2,2,2> | <4,1,4>
    shapes += [(16257, 130, 512, 0, 0), (16257, 128, 512, 0, 1), (16384, 128, 512, 32, 0)]  # 128-row tile refused: scalar A loads
    shapes += [(32704, 128, 128, 0, 0), (32705, 128, 128, 0, 0)]                        # one column of tiles: 64-row tile
    out = []
    for i, (rows, cin, cout, pool, xoff) in enumerate(shapes):
        relu = 1 if pool > 32 else (i + rows) % 2
        bias = (i // 2 + cin) % 2
        out.append(_case("linear", linear_impl(rows, cin, cout, pool, not xoff, False, bias, relu), cin, 2, 2, start=2,
                         rows=rows, cin=cin, cout=cout, pool=pool, xoff=xoff, relu=relu, bias=bias))
        if pool == 0:
            a, b = stats_mag(cin)
            out.append(_case("bn_stats", linear_impl(rows, cin, cout, 0, not xoff, True), cin, a, b, stats="y",
                             rows=rows, cin=cin, cout=cout, xoff=xoff, finish=(0, 1, 2)[i % 3]))
    return out


def xf_cases():
    out = []
    for i, (rows, cin, cout) in enumerate((r, k, c) for r in (2049, 2111, 4097) for k in (4, 36, 100, 132) for c in (32, 64, 128, 256)):
        out.append(_case("xf", linear_bn_stats_xf_impl(rows, cin, cout), cin, AMAX["xf"], 1, stats="y", rows=rows, cin=cin,
                         cout=cout, a_relu=i % 2, finish=(0, 1, 2)[i % 3]))
    out.append(_case("xf", linear_bn_stats_xf_impl(32705, 36, 128), 36, AMAX["xf"], 1, stats="y", rows=32705, cin=36, cout=128,
                     a_relu=1, finish=0))   # the 64-row tile with the transform
    out.append(_case("xf", linear_bn_stats_xf_impl(32704, 36, 128), 36, AMAX["xf"], 1, stats="y", rows=32704, cin=36, cout=128,
                     a_relu=1, finish=0))
    for rows, cin, cout in ((2048, 36, 32), (2049, 34, 32)):
        out.append(_case("xf", linear_bn_stats_xf_impl(rows, cin, cout), cin, AMAX["xf"], 1, stats="y", rows=rows, cin=cin,
                         cout=cout, a_relu=1, finish=0))
    return out


NARROW_PAIRS = [(32, 32), (32, 64), (32, 128), (64, 32), (64, 64), (64, 128), (128, 128)]


def stream_cases():
    """the streaming forward at its row threshold; rows 65535 / 65504 take the tiled kernel"""
    out = []
    for cin, cout in NARROW_PAIRS:
        for rows in (65536, 65568, 65535, 65504):
            for xf, fin in ((0, 1), (0, 2), (1, 1), (1, 2)):
                if rows < STREAM_MIN_ROWS and fin != 1 + (rows // 32 + xf) % 2:
                    continue   # the tiled kernel below the threshold: one finish per form
                if xf:
                    out.append(_case("xf", linear_bn_stats_xf_impl(rows, cin, cout), cin, AMAX["xf"], 1, stats="y", rows=rows,
                                     cin=cin, cout=cout, a_relu=1, finish=fin))
                else:
                    a, b = stats_mag(cin)
                    out.append(_case("bn_stats", linear_impl(rows, cin, cout, 0, True, True), cin, a, b, stats="y", rows=rows,
                                     cin=cin, cout=cout, xoff=0, finish=fin))
    return out


def dgrad_cases():
    out = []
    for k in range(1, 17):                       # small K: both variants
        for n_in, dxoff in [(4, 0), (128, 0), (1024, 0), (6, 0), (12, 0), (67, 0), (131, 0), (128, 1)]:
            for rows in (1, 255, 257):
                out.append(_case("dgrad", linear_dgrad_impl(rows, n_in, k, dx_aligned=not dxoff), k, 2, 2, rows=rows, n_in=n_in,
                                 n_out=k, dxoff=dxoff))
    out.append(_case("dgrad", linear_dgrad_impl(33000, 128, 9), 9, 2, 2, rows=33000, n_in=128, n_out=9, dxoff=0))
    out.append(_case("dgrad", linear_dgrad_impl(64000, 131, 9), 9, 2, 2, rows=64000, n_in=131, n_out=9, dxoff=0))
    for n_in in (1, 32, 33, 64, 65, 96, 97, 129, 260):   # MFMA forms
        for n_out in (17, 20, 33, 36, 128):
            for rows in (1, 127, 129):
                out.append(_case("dgrad", linear_dgrad_impl(rows, n_in, n_out), n_out, 2, 2, rows=rows, n_in=n_in, n_out=n_out,
                                 dxoff=0))
    for rows in (16320, 16321):
        for n_in in (129, 256):
            for n_out in (36, 33):
                out.append(_case("dgrad", linear_dgrad_impl(rows, n_in, n_out), n_out, 2, 2, rows=rows, n_in=n_in, n_out=n_out,
                                 dxoff=0))
    out.append(_case("dgrad", linear_dgrad_impl(129, 33, 36, aligned=False), 36, 2, 2, rows=129, n_in=33, n_out=36, dxoff=0,
                     dyoff=1))
    for n_in in (33, 129):   # dy given, with the sums for the layer below: pn2_linear_dgrad_bn_grad_stats (0) / pn2_linear_dgrad_fin
        for n_out in (33, 36):
            for rows in (127, 129):
                for fin in (0, 1, 3):
                    out.append(_case("dgrad", linear_dgrad_impl(rows, n_in, n_out), n_out, 2, 2, stats="g", rows=rows, n_in=n_in,
                                     n_out=n_out, dxoff=0, finish_below=fin, relu_below=(rows + fin) % 2))
    return out


def dgrad_gx_cases():
    """pn2_linear_dgrad_gx / pn2_linear_dgrad_fin with dy formed on load"""
    out = []
    i = 0
    for n_out in (20, 36, 100, 512):
        for pool, rowset in ((0, (33, 129)), (32, (32, 96, 160))):
            for rows in rowset:
                for n_in, fin in ((20, None), (20, 0), (33, 1), (129, 3), (33, None), (129, 0), (80, 1)):
                    i += 1
                    form = "gxp" if pool else "gx"
                    out.append(_case("dgrad_gx", linear_dgrad_impl(rows, n_in, n_out, gx=1, pool=pool), n_out, AMAX[form], 1,
                                     stats=None if fin is None else "g", rows=rows, n_in=n_in, n_out=n_out, pool=pool,
                                     relu=i % 2, relu_below=(i // 2) % 2, finish_below=fin))
    for rows in (16320, 16321):   # the 64-row tile with the on-load operand: its last workgroup runs past rows / 32 (pool)
        for pool in (0, 32):
            r = rows if not pool or rows % 32 == 0 else 16352   # 511 groups: the last 64-row workgroup holds one
            out.append(_case("dgrad_gx", linear_dgrad_impl(r, 129, 36, gx=1, pool=pool), 36, AMAX["gxp" if pool else "gx"], 1,
                             stats="g", rows=r, n_in=129, n_out=36, pool=pool, relu=1, relu_below=1, finish_below=1))
    for n_out in (16, 18, 516):
        out.append(_case("dgrad_gx", linear_dgrad_impl(64, 33, n_out, gx=1), n_out, AMAX["gx"], 1, rows=64, n_in=33, n_out=n_out,
                         pool=0, relu=1, relu_below=0, finish_below=None))
    return out


def dgrad_wide_cases():
    out = []
    for n_in in (64, 128):
        for rows in (65536, 65568, 65504):
            for pool in (0, 32):
                out.append(_case("dgrad_gx", linear_dgrad_impl(rows, n_in, 128, gx=1, pool=pool), 128, AMAX["gxp" if pool else "gx"],
                                 1, stats="g", rows=rows, n_in=n_in, n_out=128, pool=pool, relu=1, relu_below=1,
                                 finish_below=(1, 3)[pool // 32]))
    return out


def wgrad_cases():
    out = []
    for cin in (1, 32, 33, 67):
        for cout in (1, 32, 33, 64, 65, 131):
            rowset = [1, 2, 31] + [wgrad_rows_with(cin, cout, live) for live in (1, 2, 3, 4)]
            rowset.append(wgrad_rows_with(cin, cout, 2, last_rows=2))
            for j, rows in enumerate(rowset):
                acc = j % 2
                out.append(_case("wgrad", linear_wgrad_impl(rows, cin, cout), rows, 2, 2, start=3 * acc, rows=rows, cin=cin,
                                 cout=cout, accumulate=acc))
    # a chunk above the minimum (rows / waves > 32) with a one-row last chunk
    for cin, cout in ((32, 32), (67, 131)):
        p = wgrad_plan(40000, cin, cout)
        rows = wgrad_rows_with(cin, cout, 1, lo=40000, hi=60000) if p["chunk"] > 32 else 40001
        out.append(_case("wgrad", linear_wgrad_impl(rows, cin, cout), rows, 2, 2, rows=rows, cin=cin, cout=cout, accumulate=0))
    for rows in (65535, 65536, 65537, wgrad_rows_with(128, 128, 1, lo=65538, hi=82000)):   # eight waves from 65536 rows on
        out.append(_case("wgrad", linear_wgrad_impl(rows, 128, 128), rows, 2, 2, start=3, rows=rows, cin=128, cout=128,
                         accumulate=1))
    return out


def wgrad_onload_cases():
    """pn2_linear_wgrad_accumulate_xf / pn2_linear_wgrad_gx"""
    out = []
    i = 0
    for cin in (20, 36, 100):        # with cin 20 and cout 100: all six tile shapes
        for cout in (20, 36, 100):
            for pool in (0, 32):
                for xf in (0, 1):
                    for live in (1, 3):
                        i += 1
                        rows = wgrad_rows_with(cin, cout, live) if not pool else wgrad_rows_with(cin, cout, live, last_rows=32)
                        form = "gxp" if pool else "gx"
                        out.append(_case("wgrad_gx", linear_wgrad_impl(rows, cin, cout, xf, 2 if pool else 1), rows,
                                         AMAX["xf"] if xf else 2, AMAX[form], start=3, rows=rows, cin=cin, cout=cout, pool=pool,
                                         xf=xf, relu=i % 2, a_relu=(i // 2) % 2))
    for cin, cout in ((20, 20), (20, 36), (20, 100), (36, 20), (100, 36), (36, 100)):
        for live in (1, 2):
            rows = wgrad_rows_with(cin, cout, live)
            out.append(_case("wgrad_xf", linear_wgrad_impl(rows, cin, cout, True), rows, AMAX["xf"], 2, start=3, rows=rows, cin=cin,
                             cout=cout, a_relu=live % 2))
    for rows, pool, xf in ((65536, 0, 1), (65561, 0, 1), (65568, 32, 1), (65561, 0, 0), (65568, 32, 0)):   # eight waves
        out.append(_case("wgrad_gx", linear_wgrad_impl(rows, 128, 128, bool(xf), 2 if pool else 1), rows, AMAX["xf"] if xf else 2,
                         AMAX["gxp" if pool else "gx"], start=3, rows=rows, cin=128, cout=128, pool=pool, xf=xf, relu=1, a_relu=1))
    out.append(_case("wgrad_xf", linear_wgrad_impl(65561, 128, 128, True), 65561, AMAX["xf"], 2, start=3, rows=65561, cin=128,
                     cout=128, a_relu=1))
    return out


def fused_cases():
    out = []
    i = 0
    for cin in (32, 64):
        for cout in (32, 64):
            for rows in (32, 96, 2080):
                for pool in (0, 32):
                    for xf in (0, 1):
                        i += 1
                        form = "gxp" if pool else "gx"
                        fin = (None, 0, 1, 3)[i % 4]
                        a_mag = AMAX["xf"] if xf else 2
                        out.append(_case("fused", linear_bwd_fused(rows, cin, cout, pool), cout, AMAX[form], 1,
                                         stats=None if fin is None else "g", more=[(rows, a_mag, AMAX[form], 3, None)],
                                         rows=rows, cin=cin, cout=cout, pool=pool, xf=xf, relu=i % 2, a_relu=(i // 2) % 2,
                                         relu_below=(i // 4) % 2, finish_below=fin))
    for rows, cin, cout in ((64, 48, 32), (64, 32, 96), (33, 32, 32)):
        out.append(_case("fused", linear_bwd_fused(rows, cin, cout, 0), cout, AMAX["gx"], 1, rows=rows, cin=cin, cout=cout, pool=0,
                         xf=0, relu=1, a_relu=0, relu_below=0, finish_below=None))
    return out


def _general(rs, shape):
    """random normal data whose first channel has |mean| >> std"""
    a = rs.randn(*shape)
    if len(shape) == 2:
        a[:, 0] += 100.0
    return a.astype(F32)


def make_operands(c, rows=None, general=False):
    """general = False: the integer operands of case c (optionally at another row count) -> dict of float32 arrays.  Always: the operand pair
    the contraction sees.  linear / bn_stats / xf: a (rows, cin), w.  dgrad / dgrad_gx / fused: dy (rows, n_out), w (n_in,
    n_out).  wgrad* / fused: a (rows, cin), dy (rows, cout), dw0.  Beside them the raw tensors the entry point reads.
    general = True: the same tensors from random normal data (one channel far from zero), the formed operands through the
    float32 restatements -- for the gamma_bound test."""
    kind = c["kind"]
    rows = c["rows"] if rows is None else rows
    rs = np.random.RandomState((rows * 31 + sum(c.get(k) or 0 for k in ("cin", "cout", "n_in", "n_out", "pool"))) % (1 << 31))
    o = dict(rows=rows)
    ints_ = ints
    if general:
        ints_ = lambda rs_, shape, mag: _general(rs_, shape)

    def gx_side(width):
        if general:
            o["coef"] = np.stack([0.5 + rs.rand(width), 0.2 * rs.randn(width), 0.1 * rs.randn(width), 0.5 + rs.rand(width),
                                  0.01 * rs.randn(width), 0.01 * rs.randn(width)]).astype(F32)
            o["y"] = _general(rs, (rows, width))
            if c["pool"]:
                o["zmax"], o["ties"] = pooled_max_ties32(o["y"], o["coef"], c["relu"])
                o["dz"] = rs.randn(rows // 32, width).astype(F32)
                o["dy"] = grad_element_pooled32(o["y"], o["dz"], o["zmax"], o["ties"], o["coef"], c["relu"])
            else:
                o["dz"] = rs.randn(rows, width).astype(F32)
                o["dy"] = grad_element32(o["y"], o["dz"], o["coef"], c["relu"])
        elif c["pool"]:
            o["y"], o["dz"], o["zmax"], o["ties"], o["coef"], o["dy"] = make_gx_pooled(rs, rows, width, c["relu"])
        else:
            o["y"], o["dz"], o["coef"], o["dy"] = make_gx(rs, rows, width, c["relu"])

    def a_side(width, xf, a_relu):
        if xf and general:
            o["x"], o["sc"], o["sh"] = _general(rs, (rows, width)), (0.5 + rs.rand(width)).astype(F32), (0.2 * rs.randn(width)).astype(F32)
            o["a"] = load_transform32(o["x"], o["sc"], o["sh"], a_relu)
        elif xf:
            o["x"], o["sc"], o["sh"] = make_xf(rs, rows, width)
            o["a"] = load_transform32(o["x"], o["sc"], o["sh"], a_relu)
            assert np.abs(o["a"]).max() <= AMAX["xf"]
        else:
            o["x"] = o["a"] = ints_(rs, (rows, width), c["amax"] if kind in ("linear", "bn_stats") else 2)

    if kind in ("linear", "bn_stats", "xf"):
        a_side(c["cin"], kind == "xf", c.get("a_relu"))
        o["w"] = ints_(rs, (c["cin"], c["cout"]), c["bmax"])
        o["bias"] = ints_(rs, (c["cout"],), 2) if c.get("bias") else None
    elif kind == "dgrad":
        o["dy"] = ints_(rs, (rows, c["n_out"]), 2)
        o["w"] = ints_(rs, (c["n_in"], c["n_out"]), 2)
        if c.get("finish_below") is not None:
            o["below"] = make_below(rs, rows, c["n_in"])
    elif kind == "dgrad_gx":
        gx_side(c["n_out"])
        o["w"] = ints_(rs, (c["n_in"], c["n_out"]), 1)
        if c["finish_below"] is not None:
            o["below"] = make_below(rs, rows, c["n_in"])
    elif kind in ("wgrad", "wgrad_xf", "wgrad_gx"):
        a_side(c["cin"], kind == "wgrad_xf" or c.get("xf"), c.get("a_relu"))
        if kind == "wgrad_gx":
            gx_side(c["cout"])
        else:
            o["dy"] = ints_(rs, (rows, c["cout"]), 2)
        o["dw0"] = ints_(rs, (c["cin"], c["cout"]), 3) if c.get("accumulate", 1) else None
    elif kind == "fused":
        a_side(c["cin"], c["xf"], c["a_relu"])
        gx_side(c["cout"])
        o["w"] = ints_(rs, (c["cin"], c["cout"]), 1)
        o["dw0"] = ints_(rs, (c["cin"], c["cout"]), 3)
        if c["finish_below"] is not None:
            o["below"] = make_below(rs, rows, c["cin"])
    else:
        raise ValueError(kind)
    return o


def branch_universe():
    """every branch name the mirrors can return for a supported call: one per kernel instantiation the shipped dispatch reaches
    (tile shape x form of the A operand), plus the scalar transposed-B load of the data gradient"""
    u = {"EUNSUP"}
    u |= {"splitk<1,1,2>" + t for t in ("/vec", "/scalar")}
    u |= {"lds" + n + t for n in ("<2,2,2>", "<1,4,1>", "<1,2,1,2>/cout%128", "<1,2,1,2>/cout%64", "<4,1,2>", "<4,1,1>")
          for t in ("/vec", "/scalar")} | {"lds<4,1,4>/vec"}
    u |= {"fwd_narrow<%d,%d>%s" % (a, b, x) for a, b in NARROW_PAIRS for x in ("", "/xf")}
    u |= {"xf<2,2,2>", "xf<1,4,1>", "xf<4,1,2>", "xf<4,1,1>"}
    u |= {"smallk<%d>/%s" % (k, v) for k in range(1, 17) for v in ("reg", "lds")} | {"smallk<9>/reg/capped", "smallk<9>/lds/capped"}
    u |= {"dgrad" + n + a for n in ("<4,1,1>", "<4,1,2>", "<4,1,1>x3", "<2,2,2>", "<1,4,1>")
          for a in ("/vec/b4", "/scalar/b1", "/gx1/b4", "/gx2/b4")} | {"dgrad<4,1,2>/scalar/b4"}
    u |= {"dgrad_wide<%d>/gx%d" % (n, g) for n in (64, 128) for g in (1, 2)}
    forms = ("", "/xf", "/gx1", "/gx2", "/xf/gx1", "/xf/gx2")
    u |= {"wgrad<%d,%d>/4%s" % (a, b, f) for a in (1, 2) for b in (1, 2, 4) for f in forms} | {"wgrad<2,4>/8" + f for f in forms}
    u |= {"bwd_narrow<%d,%d>/gx%d" % (a, b, g) for a in (1, 2) for b in (1, 2) for g in (1, 2)}
    return u


def all_cases():
    return (forward_cases() + xf_cases() + stream_cases() + dgrad_cases() + dgrad_gx_cases() + dgrad_wide_cases() + wgrad_cases()
            + wgrad_onload_cases() + fused_cases())
