"""The dense-layer GEMM family (csrc/pn2_linear.hip, pn2_fwd_narrow.h, pn2_dgrad_wide.h, pn2_bwd_fused.hip) at its tile edges,
exactly: with the small-integer operands of tests/gemm_ref.py every product and every partial sum is an integer below 2^24, so
every summation order, split-K reduction and float atomic gives the same bits and each kernel must equal the int64 reference bit
for bit.  The C entry points are called directly.  Every operand is a view into the middle of a larger allocation whose slack is
NaN, every output a view into one whose slack (and initial content) is a sentinel bit pattern; after each call
  1. the output equals the integer reference,
  2. it holds no NaN (no element outside an operand entered the arithmetic),
  3. the sentinels around it are untouched (no stray store).
The cases, the branch each takes and the proof that each is exact come from gemm_ref (checked in test_gemm_edges_cpu.py).
One test repeats one case per branch with random normal data against float64 within gamma_k * (|A| . |B|)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as B  # noqa: E402
import gemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENT32, SENT64 = 0x7B5A7B5A, 0x7B5A7B5A7B5A7B5A   # finite as float32 / float64
EPS = 1e-3


def _pad(shape):
    """slack on each side, in elements: more than the 128 rows a tile can run past the end; a multiple of 64 (alignment kept)"""
    return (256 + 130 * shape[-1] + 63) // 64 * 64 if len(shape) == 2 else 1024


def gin(a, dev, off=0):
    """operand a (numpy float32, None -> None) -> device view, `off` floats off the 16-byte boundary, NaN all around"""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32)
    pad = _pad(a.shape)
    buf = torch.full((2 * pad + a.size + 8,), float("nan"), dtype=torch.float32, device=dev)
    v = buf[pad + off:pad + off + a.size]
    v.copy_(torch.from_numpy(a.reshape(-1)))
    return v.view(a.shape)


class Out:
    """output of `shape` inside a larger allocation filled with the sentinel (the output itself too, unless zero / value)"""
    def __init__(self, dev, shape, off=0, f64=False, zero=False, value=None):
        import torch
        n = int(np.prod(shape))
        pad = _pad(shape)
        self.sent = SENT64 if f64 else SENT32
        self.raw = torch.full((2 * pad + n + 8,), self.sent, dtype=torch.int64 if f64 else torch.int32, device=dev)
        self.lo, self.hi = pad + off, pad + off + n
        self.t = self.raw.view(torch.float64 if f64 else torch.float32)[self.lo:self.hi].view(shape)
        if zero:
            self.t.zero_()
        if value is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(value, np.float32)))

    def intact(self):
        return bool(((self.raw[:self.lo] == self.sent).all() & (self.raw[self.hi:] == self.sent).all()).item())

    def untouched(self):
        return bool((self.raw == self.sent).all().item())


def _mm_for(dev, work):
    """int64 matmul: numpy for small problems, float64 on the device (exact below 2^53) for large ones"""
    import torch
    if work <= 3e7:
        return R.int_mm

    def mm(a, b):
        r = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).double() @ torch.from_numpy(
            np.ascontiguousarray(b, np.float32)).to(dev).double()
        return np.rint(r.cpu().numpy()).astype(np.int64)
    return mm


def _trust(c, a, b):
    """before equality is trusted: the case is proved exact, and the operands drawn are inside the magnitudes of the proof"""
    assert all(R.exact_bound_ok(*bd) for bd in c["bounds"]), c["bounds"]
    assert np.abs(a).max() <= c["amax"] and np.abs(b).max() <= c["bmax"], (c["kind"], c["rows"])


def _exact(out, ref, what):
    """the three assertions on one output (Out) against an integer reference"""
    import torch
    got = out.t
    assert not bool(torch.isnan(got).any().item()), what + ": NaN in the output"
    g = got.detach().cpu().numpy().astype(np.float64)
    ref = np.asarray(ref, np.float64).reshape(g.shape)
    if not np.array_equal(g, ref):
        bad = np.argwhere(g != ref)
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r"
                             % (what, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], ref[tuple(bad[0])]))
    assert out.intact(), what + ": store outside the output"


def _within(out, ref64, bound, what):
    """general data: |got - ref| <= bound elementwise, no NaN, sentinels intact"""
    import torch
    assert not bool(torch.isnan(out.t).any().item()), what + ": NaN in the output"
    err = np.abs(out.t.detach().cpu().numpy().astype(np.float64) - ref64)
    assert np.all(err <= bound), "%s: error %g at bound %g" % (what, (err - bound).max(), bound.flat[(err - bound).argmax()])
    assert out.intact(), what + ": store outside the output"


def _ws(pn2, dev, c):
    nbytes = pn2._lib.lib.pn2_bn_workspace_bytes(c)
    assert nbytes == 8 * (R.BN_HEAD + (1 + R.BN_SLOTS) * 2 * c)
    return Out(dev, (nbytes // 8,), f64=True, zero=True), nbytes


def _sums(ws, c, finish, ref, what):
    """the slot copies of the per-channel sums (and, finished, their fold) against the integer reference (2, c)"""
    assert ws.intact(), what + ": store outside the workspace"
    w = ws.t.detach().cpu().numpy()
    slots = w[R.BN_HEAD + 2 * c:].reshape(R.BN_SLOTS, 2, c).sum(axis=0)
    assert np.array_equal(slots, np.asarray(ref, np.float64)), what + ": column sums"
    if finish:
        assert np.array_equal(w[R.BN_HEAD:R.BN_HEAD + 2 * c].reshape(2, c), np.asarray(ref, np.float64)), what + ": folded sums"


def _call(pn2, name, *args):
    L = pn2._lib
    return getattr(L.lib, name)(*(L.ptr(a.t if isinstance(a, Out) else a) if (hasattr(a, "data_ptr") or isinstance(a, Out) or a is None)
                                  else a for a in args), L.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------ forward
def run_forward(pn2, dev, c, general=False):
    rows, cin, cout = c["rows"], c["cin"], c["cout"]
    what = "%s %dx%d->%d %s" % (c["kind"], rows, cin, cout, c["branch"])
    o = R.make_operands(c, general=general)
    mm = _mm_for(dev, rows * cin * cout)
    x, w = gin(o["x"], dev, c.get("xoff", 0)), gin(o["w"], dev)
    if c["kind"] == "linear":
        pool, relu = c["pool"], c["relu"]
        y = Out(dev, (rows // pool if pool > 1 else rows, cout))
        rc = _call(pn2, "pn2_linear", rows, cin, cout, x, w, gin(o["bias"], dev), relu, pool, y)
        assert rc == 0, (what, rc)
        if general:
            a64, w64 = o["a"].astype(np.float64), o["w"].astype(np.float64)
            ref = a64 @ w64 + (o["bias"].astype(np.float64) if o["bias"] is not None else 0.0)
            bound = R.gamma_k(cin + 1) * (np.abs(a64) @ np.abs(w64) + (np.abs(o["bias"]) if o["bias"] is not None else 0.0))
            ref = np.maximum(ref, 0.0) if relu else ref    # ReLU and the maximum are 1-Lipschitz: the bound passes through
            if pool > 1:
                ref, bound = (t.reshape(-1, pool, cout).max(axis=1) for t in (ref, bound))
            return _within(y, ref, bound, what)
        _trust(c, o["a"], o["w"])
        return _exact(y, R.ref_forward(o["a"], o["w"], o["bias"], relu, pool, mm)[1], what)
    xf, finish = c["kind"] == "xf", c["finish"]
    sc, sh = (gin(o["sc"], dev), gin(o["sh"], dev)) if xf else (None, None)
    y = Out(dev, (rows, cout))
    ws, nbytes = _ws(pn2, dev, cout)
    rs = np.random.RandomState(cout)
    gamma, beta = rs.choice([-1.0, 1.0, 2.0], size=cout).astype(np.float32), rs.randint(-1, 2, cout).astype(np.float32)
    fin = [Out(dev, (cout,)) for _ in range(4)] if finish == 2 else [None] * 4   # save_mean, save_invstd, scale, shift
    if finish == 0 and not xf:
        rc = _call(pn2, "pn2_linear_bn_stats", rows, cin, cout, x, w, y, ws, nbytes)
    elif finish == 0:
        rc = _call(pn2, "pn2_linear_bn_stats_xf", rows, cin, cout, x, w, y, ws, nbytes, sc, sh, c["a_relu"])
    else:
        rc = _call(pn2, "pn2_linear_bn_stats_fin", rows, cin, cout, x, w, y, ws, nbytes, sc, sh, c.get("a_relu", 0), finish,
                   gin(gamma, dev) if finish == 2 else None, gin(beta, dev) if finish == 2 else None, None, EPS, 0.5, None, None,
                   *fin)
    if c["branch"] == "EUNSUP":
        assert rc == pn2._lib.PN2_EUNSUP, (what, rc)
        assert y.untouched() and ws.intact() and not bool(ws.t.any().item()), what + ": a refused call wrote"
        return
    assert rc == 0, (what, rc)
    if general:
        a64, w64 = o["a"].astype(np.float64), o["w"].astype(np.float64)
        return _within(y, a64 @ w64, R.gamma_bound(cin, np.abs(a64), np.abs(w64)), what)
    _trust(c, o["a"], o["w"])
    acc = R.ref_forward(o["a"], o["w"], mm=mm)[0]
    _exact(y, acc, what)
    s1, s2 = R.ref_column_stats(acc)
    _sums(ws, cout, finish, np.stack([s1, s2]), what)
    if finish == 2:
        # pn2_bn_finish kind 2 in float64: mean = fl32(s1 * (1 / n)) is reproducible on the host; 1 / sqrt(var + eps) goes through
        # the device's float64 square root and division before it is rounded to float32, so invstd is held to 1 float32 ulp and
        # scale / shift are derived from the moments that were published
        inv_n = 1.0 / rows
        mean_d = s1 * inv_n
        var_d = np.maximum(s2 * inv_n - mean_d * mean_d, 0.0)
        mean, invstd, scale, shift = (f.t.cpu().numpy() for f in fin)
        assert np.array_equal(mean, B.f32(mean_d)), what + ": save_mean"
        assert np.all(B.ulps(invstd, 1.0 / np.sqrt(var_d + float(np.float32(EPS)))) <= 1.0), what + ": save_invstd"
        esc, esh = B.scale_shift32(gamma, beta, mean, invstd)
        assert np.array_equal(scale, esc) and np.array_equal(shift, esh), what + ": scale / shift"
        assert all(f.intact() for f in fin)


def _by(cases, key):
    groups = {}
    for c in cases:
        groups.setdefault(key(c), []).append(c)
    return groups


FWD = _by(R.forward_cases(), lambda c: "%s-%s" % (c["branch"].replace("/vec", "").replace("/scalar", ""), c["kind"]))


@pytest.mark.parametrize("group", sorted(FWD))
def test_forward_tiles_equal_the_integer_reference(pn2, cuda, group):
    """pn2_linear (bias / ReLU / max over 16, 32, 64, 96 rows) and pn2_linear_bn_stats[_fin] on both sides of every row and column
    threshold of linear_impl, ragged rows, contraction widths 1 .. 132 that are no multiple of 4 or of 32, x on and off the 16-byte
    boundary; the column sums of y and y * y exactly at every ragged row count."""
    for c in FWD[group]:
        run_forward(pn2, cuda, c)


XFC = _by(R.xf_cases(), lambda c: c["branch"])


@pytest.mark.parametrize("group", sorted(XFC))
def test_load_transform_tiles_equal_the_integer_reference(pn2, cuda, group):
    """pn2_linear_bn_stats_xf (also through _fin): a = relu?(fma(x, scale, shift)) with shift > 0 in every channel, so a padded row
    that escaped the `live` mask of store_tile would add to the column sums; contraction widths that are multiples of 4 but not of
    32; rows <= 2048 and cin % 4 != 0 are refused and write nothing."""
    for c in XFC[group]:
        run_forward(pn2, cuda, c)


@pytest.mark.parametrize("cin,cout", R.NARROW_PAIRS)
def test_streaming_forward_and_the_tiled_kernel_below_its_threshold(pn2, cuda, cin, cout):
    """fwd_narrow_fits: rows 65536 and 65568 take the streaming kernel, 65535 and 65504 the tiled one; with and without the load
    transform, finish 1 and 2; all equal the same integer reference."""
    cases = [c for c in R.stream_cases() if (c["cin"], c["cout"]) == (cin, cout)]
    assert {c["branch"].split("<")[0] for c in cases} == {"fwd_narrow", "lds", "xf"}
    for c in cases:
        run_forward(pn2, cuda, c)


# ------------------------------------------------------------------------------------------------------------ data gradient
def _below(pn2, dev, o, c, n_in):
    """operands of the epilogue for the layer below -> (argument list, workspace, outputs of finish 3)"""
    fin = c["finish_below"]
    if fin is None:
        return [None] * 5 + [0, None, 0], None, [None] * 3
    ws, nbytes = _ws(pn2, dev, n_in)
    outs = [Out(dev, (6, n_in)), Out(dev, (n_in,)), Out(dev, (n_in,))] if fin == 3 else [None] * 3
    return [gin(a, dev) for a in o["below"]] + [c["relu_below"], ws, nbytes], ws, outs


def _check_below(o, c, n_in, dx_ref, ws, outs, what):
    fin = c.get("finish_below")
    if fin is None:
        return
    s1, s2 = R.ref_grad_stats(dx_ref, o["below"], c["relu_below"])
    _sums(ws, n_in, fin, np.stack([s1, s2]), what + " (sums for the layer below)")
    if fin == 3:   # pn2_bn_finish kind 3: coef (6, c) = sc, sh, mean, invstd, fl(s1 / n), fl(s2 / n); dgamma = fl(s2), dbeta = fl(s1)
        _, gamma, beta, mean, invstd = o["below"]
        sc, sh = B.scale_shift32(gamma, beta, mean, invstd)
        inv_n = 1.0 / o["rows"]
        coef = np.stack([sc, sh, mean, invstd, B.f32(s1 * inv_n), B.f32(s2 * inv_n)])
        assert np.array_equal(outs[0].t.cpu().numpy(), coef), what + ": coef_below"
        assert np.array_equal(outs[1].t.cpu().numpy(), B.f32(s2)) and np.array_equal(outs[2].t.cpu().numpy(), B.f32(s1)), what
        assert all(t.intact() for t in outs)


def _gx_args(dev, o, c):
    """y, dz, coef, relu, pool, zmax, ties"""
    return [gin(o["y"], dev), gin(o["dz"], dev), gin(o["coef"], dev), c["relu"], c["pool"], gin(o.get("zmax"), dev),
            gin(o.get("ties"), dev)]


def run_dgrad(pn2, dev, c, general=False):
    rows, n_in, n_out = c["rows"], c["n_in"], c["n_out"]
    what = "%s %dx%d<-%d %s" % (c["kind"], rows, n_in, n_out, c["branch"])
    o = R.make_operands(c, general=general)
    mm = _mm_for(dev, rows * n_in * n_out)
    w = gin(o["w"], dev)
    dx = Out(dev, (rows, n_in), off=c.get("dxoff", 0))
    ws, outs = None, [None] * 3
    if c["kind"] == "dgrad" and c.get("finish_below") is None:
        rc = _call(pn2, "pn2_linear_dgrad", rows, n_in, n_out, gin(o["dy"], dev, c.get("dyoff", 0)), w, dx)
    elif c["kind"] == "dgrad":   # dy given, the sums for the layer below taken in the epilogue
        below, ws, outs = _below(pn2, dev, o, c, n_in)
        if c["finish_below"] == 0:
            rc = _call(pn2, "pn2_linear_dgrad_bn_grad_stats", rows, n_in, n_out, gin(o["dy"], dev), w, dx, *below)
        else:
            rc = _call(pn2, "pn2_linear_dgrad_fin", rows, n_in, n_out, gin(o["dy"], dev), None, None, None, 0, 0, None, None, w, dx,
                       *below, c["finish_below"], *outs)
    else:
        below, ws, outs = _below(pn2, dev, o, c, n_in)
        gx = _gx_args(dev, o, c)
        if c["finish_below"] in (None, 0):
            rc = _call(pn2, "pn2_linear_dgrad_gx", rows, n_in, n_out, *gx, w, dx, *below)
        else:
            rc = _call(pn2, "pn2_linear_dgrad_fin", rows, n_in, n_out, None, *gx, w, dx, *below, c["finish_below"], *outs)
    if c["branch"] == "EUNSUP":
        assert rc == pn2._lib.PN2_EUNSUP and dx.untouched(), (what, rc)
        return None
    assert rc == 0, (what, rc)
    if general:
        d64, w64 = o["dy"].astype(np.float64), o["w"].astype(np.float64).T
        _within(dx, d64 @ w64, R.gamma_bound(n_out, np.abs(d64), np.abs(w64)), what)
        return dx
    _trust(c, o["dy"], o["w"])
    ref = R.ref_dgrad(o["dy"], o["w"], mm)
    _exact(dx, ref, what)
    _check_below(o, c, n_in, ref, ws, outs, what)
    return dx


SMALLK = _by([c for c in R.dgrad_cases() if c["branch"].startswith("smallk")], lambda c: "k%02d" % c["n_out"])


@pytest.mark.parametrize("group", sorted(SMALLK))
def test_small_k_data_gradient_equals_the_integer_reference(pn2, cuda, group):
    """K = 1 .. 16 in the register variant (n_in 4, 128, 1024) and the LDS variant (n_in 6, 12, 67, 131, and 128 with dx off the
    16-byte boundary) at rows 1, 255, 257; K = 9 past the grid cap of each variant."""
    assert {c["branch"].split("/")[1] for c in SMALLK[group]} == {"reg", "lds"}
    for c in SMALLK[group]:
        run_dgrad(pn2, cuda, c)


DGRAD = _by([c for c in R.dgrad_cases() if not c["branch"].startswith("smallk")], lambda c: c["branch"].split("/")[0])


@pytest.mark.parametrize("group", sorted(DGRAD))
def test_mfma_data_gradient_equals_the_integer_reference(pn2, cuda, group):
    """pn2_linear_dgrad on each tile shape of linear_dgrad_impl: output widths on both sides of 32, 64, 96 and 128, contraction
    widths with 16-byte and scalar loads of dy and of the transposed weights, rows 1, 127, 129, both sides of the
    <2,2,2> / <1,4,1> row threshold, and (dy given) the sums for the layer below with finish_below 0, 1, 3."""
    for c in DGRAD[group]:
        run_dgrad(pn2, cuda, c)


DGX = _by(R.dgrad_gx_cases(), lambda c: "%s-pool%d" % (c["branch"].split("/")[0], c["pool"]))


@pytest.mark.parametrize("group", sorted(DGX))
def test_data_gradient_with_dy_formed_on_load_equals_the_integer_reference(pn2, cuda, group):
    """pn2_linear_dgrad_gx / pn2_linear_dgrad_fin: dy = pn2_bn_grad_element[_pooled] formed while the tile is staged, contraction
    widths 20, 36, 100 (multiples of 4, not of 32) and 512, ragged rows, pooled groups past the end of the last workgroup; with and
    without the sums for the layer below, finish_below 0, 1, 3; n_out 16, 18, 516 are refused and write nothing."""
    for c in DGX[group]:
        run_dgrad(pn2, cuda, c)


@pytest.mark.parametrize("n_in", [64, 128])
def test_wide_data_gradient_and_the_tiled_kernel_below_its_threshold(pn2, cuda, n_in):
    """dgrad_wide_fits: rows 65536 and 65568 take the streaming kernel, 65504 the tiled one; pool 0 and 32."""
    cases = [c for c in R.dgrad_wide_cases() if c["n_in"] == n_in]
    assert {c["branch"].split("<")[0] for c in cases} == {"dgrad_wide", "dgrad"}
    for c in cases:
        run_dgrad(pn2, cuda, c)


# ---------------------------------------------------------------------------------------------------------- weight gradient
def run_wgrad(pn2, dev, c, general=False):
    rows, cin, cout = c["rows"], c["cin"], c["cout"]
    what = "%s %d: %dx%d %s %s" % (c["kind"], rows, cin, cout, c["branch"], R.wgrad_plan(rows, cin, cout))
    o = R.make_operands(c, general=general)
    mm = _mm_for(dev, rows * cin * cout)
    x = gin(o["x"], dev)
    dw = Out(dev, (cin, cout), value=o["dw0"])
    if c["kind"] == "wgrad":
        rc = _call(pn2, "pn2_linear_wgrad_accumulate" if c["accumulate"] else "pn2_linear_wgrad", rows, cin, cout, x,
                   gin(o["dy"], dev), dw)
    elif c["kind"] == "wgrad_xf":
        rc = _call(pn2, "pn2_linear_wgrad_accumulate_xf", rows, cin, cout, x, gin(o["dy"], dev), dw, gin(o["sc"], dev),
                   gin(o["sh"], dev), c["a_relu"])
    else:
        rc = _call(pn2, "pn2_linear_wgrad_gx", rows, cin, cout, x, gin(o.get("sc"), dev), gin(o.get("sh"), dev), c["a_relu"],
                   *_gx_args(dev, o, c), dw)
    assert rc == 0, (what, rc)
    if general:
        a64, d64 = o["a"].astype(np.float64).T, o["dy"].astype(np.float64)
        d0 = o["dw0"].astype(np.float64) if o["dw0"] is not None else 0.0
        # the start value is one more term of a sum formed in any order (atomics)
        return _within(dw, a64 @ d64 + d0, R.gamma_k(rows + 1) * (np.abs(a64) @ np.abs(d64) + np.abs(d0)), what)
    _trust(c, o["a"], o["dy"])
    _exact(dw, R.ref_wgrad(o["a"], o["dy"], o["dw0"], mm), what)


WGRAD = _by(R.wgrad_cases(), lambda c: c["branch"])


@pytest.mark.parametrize("group", sorted(WGRAD))
def test_weight_gradient_chunks_equal_the_integer_reference(pn2, cuda, group):
    """pn2_linear_wgrad / _accumulate (on a non-zero integer start value) on the six tile shapes: rows 1, 2, 31, and row counts
    whose last chunk holds one row (two rows) while the last workgroup holds 1, 2, 3 or 4 live chunks -- a lost or doubled row is
    a wrong integer; the eight-wave form at 65535 (four waves), 65536, 65537 and with a one-row last chunk."""
    for c in WGRAD[group]:
        run_wgrad(pn2, cuda, c)


WGX = _by(R.wgrad_onload_cases(), lambda c: c["branch"].split("/")[0] + "/" + c["branch"].split("/")[1])


@pytest.mark.parametrize("group", sorted(WGX))
def test_weight_gradient_with_operands_formed_on_load_equals_the_integer_reference(pn2, cuda, group):
    """pn2_linear_wgrad_accumulate_xf / pn2_linear_wgrad_gx at widths 20, 36, 100 (every tile shape), pool 0 and 32, the load
    transform on and off, ragged last chunks; the eight-wave form with each operand form."""
    for c in WGX[group]:
        run_wgrad(pn2, cuda, c)


# ----------------------------------------------------------------------------------------------------------- fused backward
def run_fused(pn2, dev, c, general=False):
    import torch
    rows, cin, cout = c["rows"], c["cin"], c["cout"]
    what = "fused %d: %dx%d %s" % (rows, cin, cout, c["branch"])
    o = R.make_operands(c, general=general)
    mm = _mm_for(dev, rows * cin * cout)
    got = []
    for fused in (True, False):
        x, w = gin(o["x"], dev), gin(o["w"], dev)
        xf = [gin(o.get("sc"), dev), gin(o.get("sh"), dev), c["a_relu"]]
        gx = _gx_args(dev, o, c)
        dx, dw = Out(dev, (rows, cin)), Out(dev, (cin, cout), value=o["dw0"])
        below, ws, outs = _below(pn2, dev, o, c, cin)
        fin = c["finish_below"] or 0
        if fused:
            rc = _call(pn2, "pn2_linear_bwd_fused", rows, cin, cout, x, *xf, *gx, w, dx, dw, *below, fin, *outs)
            if c["branch"] == "EUNSUP":
                assert rc == pn2._lib.PN2_EUNSUP and dx.untouched() and dw.intact(), (what, rc)
                assert np.array_equal(dw.t.cpu().numpy(), o["dw0"])
                return
        else:   # the two launches the fused kernel replaces, on the same operands
            rc = _call(pn2, "pn2_linear_dgrad_fin", rows, cin, cout, None, *gx, w, dx, *below, fin, *outs)
            assert rc == 0, (what, rc)
            rc = _call(pn2, "pn2_linear_wgrad_gx", rows, cin, cout, x, *xf, *gx, dw)
        assert rc == 0, (what, rc)
        if general:
            d64, w64, a64 = o["dy"].astype(np.float64), o["w"].astype(np.float64).T, o["a"].astype(np.float64).T
            _within(dx, d64 @ w64, R.gamma_bound(cout, np.abs(d64), np.abs(w64)), what + " dx")
            _within(dw, a64 @ d64 + o["dw0"], R.gamma_k(rows + 1) * (np.abs(a64) @ np.abs(d64) + np.abs(o["dw0"])), what + " dw")
            return
        _trust(c, o["dy"], o["w"])
        assert np.abs(o["a"]).max() <= c["bounds"][1][1]
        ref = R.ref_dgrad(o["dy"], o["w"], mm)
        _exact(dx, ref, what + " dx fused=%s" % fused)
        _exact(dw, R.ref_wgrad(o["a"], o["dy"], o["dw0"], mm), what + " dw fused=%s" % fused)
        _check_below(o, c, cin, ref, ws, outs, what + " fused=%s" % fused)
        got.append((dx.t, dw.t))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), what


FUSED = _by(R.fused_cases(), lambda c: c["branch"])


@pytest.mark.parametrize("group", sorted(FUSED))
def test_fused_backward_equals_the_integer_reference_and_the_two_launches(pn2, cuda, group):
    """pn2_linear_bwd_fused at cin, cout in {32, 64}, rows 32, 96, 2080, pool 0 and 32, the load transform on and off, the sums for
    the layer below with finish_below 0, 1, 3: dx, dw and the sums equal the integer reference and pn2_linear_dgrad_fin +
    pn2_linear_wgrad_gx on the same operands; other widths and ragged rows are refused and write nothing."""
    for c in FUSED[group]:
        run_fused(pn2, cuda, c)


# ------------------------------------------------------------------------------------------------------------- general data
RUNNERS = {"linear": run_forward, "bn_stats": run_forward, "xf": run_forward, "dgrad": run_dgrad, "dgrad_gx": run_dgrad,
           "wgrad": run_wgrad, "wgrad_xf": run_wgrad, "wgrad_gx": run_wgrad, "fused": run_fused}


def _one_per_branch():
    seen = {}
    for c in R.all_cases():
        if c["branch"] != "EUNSUP" and (c["branch"] not in seen or c["rows"] < seen[c["branch"]]["rows"]):
            seen[c["branch"]] = c
    return _by(seen.values(), lambda c: c["kind"])


GENERAL = _one_per_branch()


@pytest.mark.parametrize("kind", sorted(GENERAL))
def test_every_branch_on_general_data_within_the_forward_error_bound(pn2, cuda, kind):
    """one case per branch with random normal operands, one channel with |mean| >> std, against float64:
    |err| <= gamma_k * (|A| . |B|) elementwise, gamma_k = k u / (1 - k u), u = 2^-24, k = contraction length + epilogue additions
    (a bound for every summation order; integer data cannot show a wrong rounding path such as a missing fma in an operand
    transform -- the formed operands here are the float32 restatements of gemm_ref)."""
    for c in GENERAL[kind]:
        RUNNERS[kind](pn2, cuda, c, general=True)


# ------------------------------------------------------------------------------------- padded elements and infinite operands
def test_an_infinite_formed_operand_gives_infinity_not_nan_through_the_padding(pn2, cuda):
    """The `live` mask of store_tile zeroes the padded part of a staged A tile AFTER the operand transform.  The B tile is zero
    there too, so with finite data a padded element that escaped the mask would still contribute 0 to the OUTPUT (only the forward
    statistics, which sum padded rows, would see it).  An infinite element makes the difference visible: the clamped re-read of
    the last channel group brings it into the padding, where inf * 0 = NaN.  Contraction width 36 (one 4-wide group past 32); the
    infinite element sits in the last channel, whose weights are all 1: its row of the output is infinite in every column, every
    other row equals the integer reference, and nothing is NaN."""
    inf = np.float32(np.inf)
    # load transform (XF)
    c = next(k for k in R.xf_cases() if (k["rows"], k["cin"], k["cout"]) == (2049, 36, 64))
    o = R.make_operands(c)
    r = 100
    o["x"][r, 35], o["sc"][35], o["w"][35, :] = inf, 1.0, 1.0
    a = R.load_transform32(o["x"], o["sc"], o["sh"], c["a_relu"])
    assert np.isinf(a).sum() == 1 and a[r, 35] == inf
    y = Out(cuda, (2049, 64))
    ws, nbytes = _ws(pn2, cuda, 64)
    rc = _call(pn2, "pn2_linear_bn_stats_xf", 2049, 36, 64, gin(o["x"], cuda), gin(o["w"], cuda), y, ws, nbytes, gin(o["sc"], cuda),
               gin(o["sh"], cuda), c["a_relu"])
    assert rc == 0, rc
    ref = R.int_mm(np.where(np.isinf(a), 0, a), o["w"]).astype(np.float64)
    ref[r, :] = np.inf
    _exact(y, ref, "load transform with an infinite element")
    sums = ws.t.cpu().numpy()[R.BN_HEAD + 2 * 64:].reshape(R.BN_SLOTS, 2, 64).sum(axis=0)
    assert np.all(sums == np.inf), "column sums of a column that holds +inf"
    # gradient formed on load (GX = 1, GX = 2)
    for pool, rows in ((0, 129), (32, 96)):
        c = dict(kind="dgrad_gx", rows=rows, n_in=33, n_out=36, pool=pool, relu=0, relu_below=0, finish_below=None)
        o = R.make_operands(c)
        o["w"][:, 35] = 1.0
        sign = float(o["coef"][0, 35])   # sc = +-1
        o["dz"][1, 35] = inf     # pool: the pooled gradient of group 1, shared by the rows that attain its maximum
        with np.errstate(invalid="ignore"):
            dy = (R.grad_element_pooled32(o["y"], o["dz"], o["zmax"], o["ties"], o["coef"], 0) if pool
                  else R.grad_element32(o["y"], o["dz"], o["coef"], 0))
        hot = np.isinf(dy).any(axis=1)
        assert not np.isnan(dy).any() and np.all(dy[hot, 35] == sign * inf) and hot.sum() == np.isinf(dy).sum() >= 1
        dx = Out(cuda, (rows, 33))
        rc = _call(pn2, "pn2_linear_dgrad_gx", rows, 33, 36, *_gx_args(cuda, o, c), gin(o["w"], cuda), dx, *([None] * 5 + [0, None, 0]))
        assert rc == 0, rc
        ref = R.ref_dgrad(np.where(np.isinf(dy), 0, dy), o["w"]).astype(np.float64)
        ref[hot, :] = sign * np.inf
        _exact(dx, ref, "gradient on load (pool %d) with an infinite element" % pool)


# ------------------------------------------------------------------------------------------------------ argument contracts
def test_argument_contracts_refuse_without_writing(pn2, cuda):
    """the contracts the source states: cout % 32, unaligned w, pool values, rows % pool, a wide pool without ReLU, null operands
    and the PN2_EUNSUP cases of each on-load form; every refusal leaves the output sentinels untouched"""
    L = pn2._lib
    K = L.ABI.constants
    rs = np.random.RandomState(0)
    x, w, w_off = gin(R.ints(rs, (2080, 36), 2), cuda), gin(R.ints(rs, (36, 64), 2), cuda), gin(R.ints(rs, (36, 64), 2), cuda, 1)
    y = Out(cuda, (2080, 64))
    lin = lambda rows, cin, cout, xx, ww, relu, pool, yy=y: _call(pn2, "pn2_linear", rows, cin, cout, xx, ww, None, relu, pool, yy)
    assert lin(2080, 36, 48, x, w, 0, 0) == K["PN2_EUNSUP"]                  # cout % 32
    assert lin(2080, 36, 64, x, w_off, 0, 0) == K["PN2_EUNSUP"]              # w off the 16-byte boundary
    assert lin(2080, 36, 64, x, w, 1, 8) == K["PN2_EUNSUP"]                  # pool neither 16 nor a multiple of 32
    assert lin(2080, 36, 64, x, w, 1, 48) == K["PN2_EUNSUP"]
    assert lin(2080, 36, 64, x, w, 1, 64) == K["PN2_EINVAL"]                 # rows % pool
    assert lin(2048, 36, 64, x, w, 0, 64) == K["PN2_EUNSUP"]                 # the atomic maximum needs the ReLU
    assert lin(0, 36, 64, x, w, 0, 0) == K["PN2_EINVAL"]
    assert lin(2080, 36, 64, None, w, 0, 0) == K["PN2_ENULL"] and lin(2080, 36, 64, x, None, 0, 0) == K["PN2_ENULL"]
    assert _call(pn2, "pn2_linear", 2080, 36, 64, x, w, None, 0, 0, None) == K["PN2_ENULL"]
    assert y.untouched()
    ws, nbytes = _ws(pn2, cuda, 64)
    assert _call(pn2, "pn2_linear_bn_stats", 2080, 36, 64, x, w, y, None, nbytes) == K["PN2_ENULL"]
    assert _call(pn2, "pn2_linear_bn_stats", 2080, 36, 64, x, w, y, ws, nbytes - 8) == K["PN2_EINVAL"]
    sc = gin(np.ones(36, np.float32), cuda)
    sc_off = gin(np.ones(36, np.float32), cuda, 1)
    xfc = lambda rows, cin, a, b: _call(pn2, "pn2_linear_bn_stats_xf", rows, cin, 64, x, w, y, ws, nbytes, a, b, 1)
    assert xfc(2080, 36, sc, None) == K["PN2_ENULL"] and xfc(2080, 36, sc, sc_off) == K["PN2_EUNSUP"]
    assert xfc(2048, 36, sc, sc) == K["PN2_EUNSUP"] and xfc(2080, 34, sc, sc) == K["PN2_EUNSUP"]
    assert _call(pn2, "pn2_linear_bn_stats_fin", 2080, 36, 64, x, w, y, ws, nbytes, None, None, 0, 3, *[None] * 3, EPS, 0.5,
                 *[None] * 6) == K["PN2_EINVAL"]                             # finish is 1 or 2
    assert _call(pn2, "pn2_linear_bn_stats_fin", 2080, 36, 64, x, w, y, ws, nbytes, None, None, 0, 2, *[None] * 3, EPS, 0.5,
                 *[None] * 6) == K["PN2_ENULL"]                              # finish 2 needs gamma, beta, save_*
    assert y.untouched() and ws.intact() and not bool(ws.t.any().item())
    # the on-load data gradient: pool values, rows % 32, null and unaligned operands
    c = dict(kind="dgrad_gx", rows=96, n_in=33, n_out=36, pool=32, relu=1, relu_below=0, finish_below=None, amax=0, bmax=1)
    o = R.make_operands(c)
    g = _gx_args(cuda, o, c)
    wt, dx = gin(o["w"], cuda), Out(cuda, (96, 33))
    nob = [None] * 5 + [0, None, 0]
    dgx = lambda rows, gg, n_out=36: _call(pn2, "pn2_linear_dgrad_gx", rows, 33, n_out, *gg, wt, dx, *nob)
    assert dgx(96, g[:4] + [16] + g[5:]) == K["PN2_EINVAL"] and dgx(80, g) == K["PN2_EINVAL"]
    assert dgx(96, g[:5] + [None, g[6]]) == K["PN2_ENULL"] and dgx(96, [None] + g[1:]) == K["PN2_ENULL"]
    assert dgx(96, [gin(o["y"], cuda, 1)] + g[1:]) == K["PN2_EUNSUP"]
    assert _call(pn2, "pn2_linear_dgrad_fin", 96, 33, 36, g[0], *g, wt, dx, *nob, 0, None, None, None) == K["PN2_EINVAL"]  # dy and y
    assert _call(pn2, "pn2_linear_dgrad_fin", 96, 33, 36, None, *g, wt, dx, *nob, 1, None, None, None) == K["PN2_EINVAL"]  # no layer below
    assert _call(pn2, "pn2_linear_dgrad", 96, 33, 36, None, wt, dx) == K["PN2_ENULL"]
    assert dx.untouched()
    dw = Out(cuda, (33, 36))
    xs = gin(R.ints(rs, (96, 33), 2), cuda)
    wgx = lambda rows, a, b, gg: _call(pn2, "pn2_linear_wgrad_gx", rows, 33, 36, xs, a, b, 1, *gg, dw)
    s33 = gin(np.ones(33, np.float32), cuda)
    assert wgx(96, s33, None, g) == K["PN2_ENULL"] and wgx(80, None, None, g) == K["PN2_EINVAL"]
    assert wgx(96, None, None, g[:4] + [64] + g[5:]) == K["PN2_EINVAL"] and wgx(96, None, None, g[:6] + [None]) == K["PN2_ENULL"]
    assert _call(pn2, "pn2_linear_wgrad_accumulate_xf", 96, 33, 36, xs, g[0], dw, s33, None, 1) == K["PN2_ENULL"]
    assert _call(pn2, "pn2_linear_wgrad", 96, 33, 36, xs, None, dw) == K["PN2_ENULL"]
    assert dw.untouched()
