"""The training-mode batch-norm kernels (csrc/pn2_bn.hip, pn2_bn_finish / bn_scale_shift in csrc/pn2_common.h) at their edges,
entry point by entry point through the C ABI: pn2_bn_relu_forward, _mode, _pool, _deferred, pn2_bn_relu_backward, _mode and
pn2_bn_grad_constants (every PN2_BN_WS_* state of the workspace) against the float64 oracle and the float32 restatement of tests/bn_ref.py.

Shapes come from the kernels' thread mapping (cv = c / vec columns, rp = 256 // cv row slots; one reduction block while
rows <= 8 * rp; two slot copies of the accumulators from 33 blocks).  Every output is a 16-byte aligned view inside a larger
tensor filled with a NaN bit pattern and the workspace is exactly pn2_bn_workspace_bytes(c) inside one: whatever a call writes
outside its view fails the call's check.  Tolerances: "bit-equal", "1 ulp" / "2 ulp" of float32, or the MEASURED bound of
bn_ref.bound -- 4 x the error of the float32 restatement (from the float64 moments rounded to float32, never from the kernel's
output) against float64 on the same input with the restatement's own ReLU mask and ties, taken per channel and floored at
1 float32 ulp of the output scale.  The docstrings give the worst measured
restatement error per test in float32 ulps of the output scale (max |reference|); every test prints a "[bn_edges]" line with
that figure and the kernel's own worst error, restatement / kernel, per output (pytest -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-3))      # the kernels take eps and decay as float32
DECAY = float(np.float32(0.9))
POISON = -0x5A5A5B                 # int32 of 0xFFA5A5A5: a NaN as float32
LEAD = 64                          # margin, in 4-byte words, on both sides of every view
EINVAL, ENULL, EUNSUP = -1, -2, -4

SPECS = {
    "pn2_bn_relu_forward": "rows c y gamma beta bias eps decay relu pool rm rv ws wsb sm si z ties stream",
    "pn2_bn_relu_forward_mode": "rows c y gamma beta bias eps decay relu rm rv ws wsb mode sm si z stream",
    "pn2_bn_relu_forward_pool": "rows c y gamma beta bias eps decay relu pool rm rv ws wsb mode sm si z ties ysel stream",
    "pn2_bn_relu_forward_deferred": "rows c y gamma beta bias eps decay stats_done rm rv ws wsb sm si scale shift stream",
    "pn2_bn_relu_backward": "rows c dz y gamma beta sm si relu pool zmax ties ws wsb dy dgamma dbeta stream",
    "pn2_bn_relu_backward_mode": "rows c dz y gamma beta sm si relu pool zmax ties ws wsb mode dy dgamma dbeta stream",
    "pn2_bn_grad_constants": "rows c dz y gamma beta sm si relu pool zmax ties ysel stats_done ws wsb coef dgamma dbeta stream",
}
FWD = "pn2_bn_relu_forward"
FWD_MODE, FWD_POOL, FWD_DEF = FWD + "_mode", FWD + "_pool", FWD + "_deferred"
BWD = "pn2_bn_relu_backward"
BWD_MODE, GCONST = BWD + "_mode", "pn2_bn_grad_constants"


# ------------------------------------------------------------------------------------------------------- guarded buffers
class Buf:
    """float32 view of `shape` inside a larger poisoned tensor, `off` floats past a 16-byte boundary"""

    def __init__(self, dev, shape, data=None, off=0):
        import torch
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.n, self.lead = int(np.prod(self.shape)), LEAD + off
        self.base = torch.full((self.lead + self.n + LEAD,), POISON, dtype=torch.int32, device=dev)
        self.t = self.base[self.lead:self.lead + self.n].view(torch.float32)
        assert self.t.data_ptr() % 16 == (4 * off) % 16
        self.init = None
        if data is not None:
            self.init = np.ascontiguousarray(data, np.float32).reshape(-1)
            assert self.init.size == self.n
            self.t.copy_(torch.from_numpy(self.init))

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def raw(self):
        """the view's words after checking that both margins still hold the poison"""
        b = self.base.cpu().numpy()
        assert (b[:self.lead] == POISON).all() and (b[self.lead + self.n:] == POISON).all(), "wrote outside its view"
        return b[self.lead:self.lead + self.n]

    def get(self):
        return self.raw().view(np.float32).reshape(self.shape).copy()

    def untouched(self):
        w = self.raw()
        return bool((w == POISON).all()) if self.init is None else np.array_equal(w, self.init.view(np.int32))


class Ws:
    """exactly pn2_bn_workspace_bytes(c) bytes, filled with 0x00 or 0xFF, with poison in front and behind"""

    def __init__(self, raw, dev, c, fill=0):
        import torch
        self.nbytes = int(raw.pn2_bn_workspace_bytes(c))
        assert self.nbytes % 8 == 0 and self.nbytes >= 2 * c * 8
        self.n, self.fill = self.nbytes // 4, (0 if fill == 0 else -1)
        self.base = torch.full((LEAD + self.n + LEAD,), POISON, dtype=torch.int32, device=dev)
        self.base[LEAD:LEAD + self.n] = self.fill
        self.t = self.base[LEAD:LEAD + self.n]
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def raw(self):
        b = self.base.cpu().numpy()
        assert (b[:LEAD] == POISON).all() and (b[LEAD + self.n:] == POISON).all(), "wrote outside the workspace"
        return b[LEAD:LEAD + self.n]

    def untouched(self):
        return bool((self.raw() == self.fill).all())


def call(raw, dev, entry, ins, outs, off=(), null=(), ws=None, ws_fill=0, alias=None, expect=0, **scalars):
    """One ABI call.  ins: name -> numpy array (uploaded into a guarded view) / Buf / None (NULL); outs: name -> shape of a
    poisoned output view; off: names whose view starts 4 bytes off a 16-byte boundary; null: names passed as NULL although
    allocated; alias: {output: input} sharing one view (dy == dz).  Asserts the return code; after a refusal, that no output,
    in-out operand or workspace word changed.  -> dict name -> numpy (outputs and the in-out moving averages), "_ws", "_bufs"."""
    import torch
    rows, c = scalars["rows"], scalars["c"]
    bufs = {}
    for name, a in ins.items():
        if a is not None:
            bufs[name] = a if isinstance(a, Buf) else Buf(dev, np.shape(a), a, off=1 if name in off else 0)
    alias = alias or {}
    for name, shape in outs.items():
        bufs[name] = bufs[alias[name]] if name in alias else Buf(dev, shape, off=1 if name in off else 0)
    ws = ws if ws is not None else Ws(raw, dev, c, ws_fill)
    before = ws.raw().copy() if expect != 0 else None
    args = []
    for name in SPECS[entry].split():
        if name == "ws":
            args.append(None if "ws" in null else ws.ptr())
        elif name == "wsb":
            args.append(ws.nbytes)
        elif name == "stream":
            args.append(None)
        elif name in scalars:
            args.append(scalars[name])
        elif name in ("eps", "decay"):
            args.append(EPS if name == "eps" else DECAY)
        else:
            args.append(None if name in null or name not in bufs else bufs[name].ptr())
    rc = getattr(raw, entry)(*args)
    torch.cuda.synchronize()
    assert rc == expect, "%s returned %d, expected %d (%s)" % (entry, rc, expect, scalars)
    res = {"_ws": ws, "_bufs": bufs}
    if expect != 0:
        for name, b in bufs.items():
            assert b.untouched(), "%s refused the call (%d) but changed %s" % (entry, rc, name)
        assert np.array_equal(ws.raw(), before), "%s refused the call (%d) but wrote to the workspace" % (entry, rc)
        return res
    ws.raw()
    for name, b in bufs.items():
        if name in outs or name in ("rm", "rv"):
            res[name] = b.get()
        elif name not in alias.values():
            assert b.untouched(), "%s changed its input %s" % (entry, name)
    return res


# ------------------------------------------------------------------------------------------------------ shapes and inputs
def mapping(c):
    vec = 4 if c % 4 == 0 else 1
    cv = c // vec
    return vec, cv, 256 // cv


def reduction_blocks(rows, c):
    """bn_plan: at most 512 blocks, each a slab of at least 8 passes of rp rows, rounded up to a multiple of rp"""
    rp = mapping(c)[2]
    slab = max(-(-rows // 512), 8 * rp)
    slab = -(-slab // rp) * rp
    return -(-rows // slab)


def sweep_rows(c):
    rp = mapping(c)[2]
    rows = [1, 2, 8 * rp, 8 * rp + 1, 33 * 8 * rp + 3]
    assert [reduction_blocks(r, c) for r in rows] == [1, 1, 1, 2, 34]      # 34 blocks: two slot copies
    return rows


def plain_input(rows, c, seed):
    rs = np.random.RandomState(seed)
    ch = np.arange(c)
    return dict(y=(rs.randn(rows, c) * (1.0 + ch % 5) + 3.0 * np.sin(ch)).astype(np.float32),
                gamma=(0.5 + rs.rand(c)).astype(np.float32), beta=(rs.randn(c) * 0.3).astype(np.float32),
                bias=rs.randn(c).astype(np.float32), dz=rs.randn(rows, c).astype(np.float32))


def pool_input(groups, pool, c, seed):
    """duplicated rows (the second half of every third group repeats its first row), a group of identical rows, channels that
    never pass the ReLU (beta = -6: every row ties at 0, with different y), and channel 1 with gamma = 0, beta = -0 and a
    positive mean: sc = 0, sh = -0, so z = -0 where y < 0 and +0 elsewhere -- all rows tie, the pooled value keeps the first
    row's sign bit.  c >= 3."""
    rs = np.random.RandomState(seed)
    y = rs.randn(groups, pool, c).astype(np.float32)
    y[:, :, 1] = np.abs(y[:, :, 1]) + 0.5        # channel 1: positive mean whatever the negatives planted below ...
    y[0, 0, 1], y[4::3, 1, 1] = -0.5, -0.25       # ... and group 0 starts on a negative value: its pooled z is -0
    y[::3, 0, 2] = 10.0                          # channel 2: the first row of every third group is its maximum, and is repeated
    y[::3, pool // 2:, :] = y[::3, :1, :]
    y[1, :, :] = y[1, :1, :]
    gamma = (0.5 + rs.rand(c)).astype(np.float32)
    beta = (rs.randn(c) * 0.3).astype(np.float32)
    beta[::5] = -6.0
    gamma[1], beta[1] = 0.0, -0.0
    return dict(y=y.reshape(groups * pool, c), gamma=gamma, beta=beta, dz=rs.randn(groups, c).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ comparisons
class Notes:
    """collects, per output, the worst restatement error and the worst kernel error in float32 ulps of the output scale"""

    def __init__(self, label):
        self.label, self.rows = label, {}

    def within(self, name, got, ref64, restated, per_channel=True, own=None):
        """|got - ref64| <= bn_ref.bound of the host restatement, measured per channel against `own`: the float64 reference that
        takes the RESTATEMENT's ReLU mask / tie pattern (ref64 may take the kernel's; default: ref64 itself)"""
        ref64 = np.asarray(ref64, np.float64)
        bound, measured = B.bound(restated, ref64 if own is None else own, per_channel)
        err = np.abs(np.asarray(got, np.float64) - ref64)
        unit = float(B.ulp32(np.abs(ref64).max()))
        w = self.rows.setdefault(name, [0.0, 0.0])
        w[0], w[1] = max(w[0], float(np.max(measured)) / unit), max(w[1], float(err.max()) / unit)
        assert (err <= bound).all(), "%s %s: kernel off by %.3g ulp of the output scale, restatement by %.3g (bound 4 x, floor 1)" % (
            self.label, name, float(np.nanmax(err)) / unit, float(np.max(measured)) / unit)

    def ulp(self, name, got, ref64, n=1.0):
        u = B.ulps(got, ref64)
        w = self.rows.setdefault(name + "[ulp]", [0.0, 0.0])
        w[1] = max(w[1], float(u.max()))
        assert (u <= n).all(), "%s %s: %.3g ulp from float64 (allowed %g)" % (self.label, name, float(np.nanmax(u)), n)

    def done(self):
        print("[bn_edges] %s: " % self.label + "; ".join("%s %.3g/%.3g" % (k, v[0], v[1]) for k, v in sorted(self.rows.items())))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def host_model(O, a, relu, pool=0, dz=None):
    """float64 reference + the restatement from the float64 moments rounded to float32 (what the bounds are measured on)"""
    fw = B.forward64(O, a["y"], a["gamma"], a["beta"], relu, EPS, pool)
    rh = B.restate(a["y"], a["gamma"], a["beta"], relu, B.f32(fw["mean"]), B.f32(fw["invstd"]), dz, pool)
    if dz is not None:
        rh["dy64"], rh["dg64"], rh["db64"] = B.backward64(O, a["y"], a["gamma"], a["beta"], dz, relu, EPS, pool, z_pattern=rh["z"])
    return fw, rh


def check_backward(nt, res, ref, rh, rows, coef_only=False, pooled=False):
    """dy / dgamma / dbeta (or coef[4:6] = k1, k2) of a kernel against the float64 `ref` = (dy, dgamma, dbeta) that takes the
    kernel's ReLU mask and tie pattern; the bounds are measured on the host restatement rh against the float64 reference with
    rh's OWN mask and ties (rh["dy64"], rh["dg64"], rh["db64"]).  pooled: the pooled reduction's restatement, without channel 1
    of pool_input (gamma = 0: rows of different y tie and the pooled form stands for them by the first; check_pool holds that
    channel to the restatement directly)."""
    sfx = "p" if pooled else ""
    sel = np.arange(len(ref[1])) != 1 if pooled else slice(None)
    nt.within("dgamma" + sfx, res["dgamma"][sel], ref[1][sel], rh["dgamma" + sfx][sel], own=rh["dg64"][sel])
    nt.within("dbeta" + sfx, res["dbeta"], ref[2], rh["dbeta" + sfx], own=rh["db64"])
    if coef_only:
        nt.within("k1" + sfx, res["coef"][4], ref[2] / rows, rh["k1" + sfx], own=rh["db64"] / rows)
        nt.within("k2" + sfx, res["coef"][5][sel], ref[1][sel] / rows, rh["k2" + sfx][sel], own=rh["dg64"][sel] / rows)
    else:
        nt.within("dy", res["dy"], ref[0], rh["dy"], own=rh["dy64"])


def check_coef_head(res, a, sm, si):
    sc, sh = B.scale_shift32(a["gamma"], a["beta"], sm, si)
    assert same_bits(res["coef"][0], sc) and same_bits(res["coef"][1], sh), "coef sc / sh differ from gamma*invstd, fma(-mean, sc, beta)"
    assert same_bits(res["coef"][2], sm) and same_bits(res["coef"][3], si)


# ================================================================================ 1. channel and row sweep, no pool
SCALAR_C = [1, 2, 3, 5, 7, 63, 255]
VECTOR_C = [4, 12, 36, 100, 260, 516, 1020, 1024]


def check_plain(raw, O, dev, rows, c, relu, nt):
    a = plain_input(rows, c, 1000 * c + rows + relu)
    y, dz = a["y"], a["dz"]
    rm0, rv0 = np.full(c, 0.25, np.float32), np.full(c, 2.0, np.float32)
    fw, rh = host_model(O, a, relu, dz=dz)
    mv = B.forward64(O, y, a["gamma"], a["beta"], relu, EPS, 0, a["bias"], (rm0, rv0), DECAY)
    base = dict(y=y, gamma=a["gamma"], beta=a["beta"])
    # forward, moving averages with decay 0.9 and the folded-away bias
    f = call(raw, dev, FWD, dict(base, bias=a["bias"], rm=rm0, rv=rv0), dict(sm=c, si=c, z=(rows, c)), rows=rows, c=c, relu=relu, pool=0)
    nt.ulp("save_mean", f["sm"], fw["mean"])
    nt.ulp("save_invstd", f["si"], fw["invstd"])
    nt.within("z", f["z"], fw["z"], rh["z"])
    nt.ulp("running_mean", f["rm"], mv["mm"])
    nt.ulp("running_var", f["rv"], mv["mv"])
    # backward: the float64 reference takes the kernel's ReLU mask
    ref = B.backward64(O, y, a["gamma"], a["beta"], dz, relu, EPS, 0, z_pattern=f["z"]) if relu else (rh["dy64"], rh["dg64"], rh["db64"])
    bin_ = dict(base, dz=dz, sm=f["sm"], si=f["si"])
    b = call(raw, dev, BWD, bin_, dict(dy=(rows, c), dgamma=c, dbeta=c), rows=rows, c=c, relu=relu, pool=0)
    check_backward(nt, b, ref, rh, rows)
    if rows == 1:
        assert not b["dy"].any() and not b["dgamma"].any(), "one row: dy and dgamma are exactly 0"
    bi = call(raw, dev, BWD, bin_, dict(dy=(rows, c), dgamma=c, dbeta=c), alias={"dy": "dz"}, rows=rows, c=c, relu=relu, pool=0)
    assert same_bits(bi["dy"], b["dy"]) and same_bits(bi["dgamma"], b["dgamma"]) and same_bits(bi["dbeta"], b["dbeta"]), "dy == dz differs"
    # deferred form (statistics taken here, workspace zeroed by the caller), moving averages with decay 0 and no bias
    d = call(raw, dev, FWD_DEF, dict(base, rm=rm0, rv=rv0), dict(sm=c, si=c, scale=c, shift=c), rows=rows, c=c, stats_done=0, decay=0.0)
    nt.ulp("save_mean", d["sm"], fw["mean"])
    nt.ulp("save_invstd", d["si"], fw["invstd"])
    sc, sh = B.scale_shift32(a["gamma"], a["beta"], d["sm"], d["si"])
    assert same_bits(d["scale"], sc) and same_bits(d["shift"], sh), "deferred scale / shift are not gamma*invstd, fma(-mean, sc, beta)"
    nt.ulp("running_mean", d["rm"], fw["mean"])
    nt.ulp("running_var", d["rv"], fw["var"] * (rows / (rows - 1.0) if rows > 1 else 1.0))
    # gradient constants (reduction taken here)
    g = call(raw, dev, GCONST, bin_, dict(coef=(6, c), dgamma=c, dbeta=c), rows=rows, c=c, relu=relu, pool=0, stats_done=0)
    check_coef_head(g, a, f["sm"], f["si"])
    check_backward(nt, g, ref, rh, rows, coef_only=True)
    if rows == 1:
        assert not g["dgamma"].any() and not g["coef"][5].any()


@pytest.mark.parametrize("ri", range(5), ids=["1row", "2rows", "1block", "1block+1", "34blocks"])
@pytest.mark.parametrize("c", SCALAR_C + VECTOR_C)
def test_channel_and_row_sweep(pn2, oracle, cuda, c, ri):
    """c in {1, 2, 3, 5, 7, 63, 255} (scalar path) and {4, 12, 36, 100, 260, 516, 1020, 1024} (16-byte path: rp = 1 at 1020 / 1024,
    idle threads where cv does not divide 256, odd reduction trees) x rows in {1, 2, 8 rp, 8 rp + 1, 33 * 8 rp + 3} (one block; a
    last block of one row; 34 blocks = two slot copies) x relu in {0, 1}: pn2_bn_relu_forward, pn2_bn_relu_backward (also with
    dy == dz, bit-equal), pn2_bn_relu_forward_deferred and pn2_bn_grad_constants.  Saved moments and moving averages (decay 0.9
    with bias; decay 0 without) within 1 ulp of float64; scale, shift, coef[0:4] bit-equal to the restatement from the saved
    moments; z, dy, k1, k2, dgamma, dbeta within the measured bound; at one row dy and dgamma are exactly 0.

    Measured restatement error, worst over the whole sweep, in ulps of the output scale: z 394 (one row: z = beta is rounded at the
    size of y * sc), dy 5.4e3 (two rows: dy is what is left of g after two cancellations), dgamma / k2 58, dbeta / k1 0.5; at 8 rp
    rows and more: z 2.5, dy 3.4, dgamma 4.2, k2 7.2, dbeta / k1 0.5.  Each case prints its own figures next to the kernel's."""
    raw = pn2._lib._raw
    rows = sweep_rows(c)[ri]
    nt = Notes("sweep c=%d rows=%d" % (c, rows))
    for relu in (0, 1):
        check_plain(raw, oracle, cuda, rows, c, relu, nt)
    nt.done()


@pytest.mark.parametrize("c", [5, 36, 1020])
def test_moving_averages(pn2, oracle, cuda, c):
    """running_mean / running_var of pn2_bn_relu_forward and pn2_bn_relu_forward_deferred at rows in {1, 8 rp + 1}: decay in
    {0, 0.9, 1} x bias given / NULL, and running_* NULL.  decay = 1 leaves them bit-unchanged; decay = 0 gives float32(mean + bias)
    and the unbiased variance (rows / (rows - 1), the biased one at a single row); all within 1 ulp of float64."""
    raw = pn2._lib._raw
    nt = Notes("moving averages c=%d" % c)
    for rows in (1, 8 * mapping(c)[2] + 1):
        a = plain_input(rows, c, 77 * c + rows)
        rm0, rv0 = (0.25 + np.arange(c) % 3).astype(np.float32), (2.0 - 0.125 * (np.arange(c) % 4)).astype(np.float32)
        base = dict(y=a["y"], gamma=a["gamma"], beta=a["beta"])
        for entry, outs, extra in ((FWD, dict(sm=c, si=c, z=(rows, c)), dict(relu=1, pool=0)),
                                   (FWD_DEF, dict(sm=c, si=c, scale=c, shift=c), dict(stats_done=0))):
            for decay in (0.0, DECAY, 1.0):
                for bias in (a["bias"], None):
                    ref = B.forward64(oracle, a["y"], a["gamma"], a["beta"], 1, EPS, 0, bias, (rm0, rv0), decay)
                    r = call(raw, cuda, entry, dict(base, bias=bias, rm=rm0, rv=rv0), outs, rows=rows, c=c, decay=decay, **extra)
                    if decay == 1.0:
                        assert same_bits(r["rm"], rm0) and same_bits(r["rv"], rv0)
                    if decay == 0.0:
                        unb = ref["var"] * (rows / (rows - 1.0) if rows > 1 else 1.0)
                        nt.ulp("running_mean", r["rm"], ref["mean"] + (0.0 if bias is None else bias.astype(np.float64)))
                        nt.ulp("running_var", r["rv"], unb)
                    nt.ulp("running_mean", r["rm"], ref["mm"])
                    nt.ulp("running_var", r["rv"], ref["mv"])
            r = call(raw, cuda, entry, dict(base, bias=a["bias"]), outs, rows=rows, c=c, **extra)   # no moving averages kept
            nt.ulp("save_mean", r["sm"], ref["mean"])
            nt.ulp("save_invstd", r["si"], ref["invstd"])
    nt.done()


# ================================================================================================== 2. pool sweep
def check_pool(raw, O, dev, groups, pool, c, relu, nt):
    rows = groups * pool
    a = pool_input(groups, pool, c, 31 * c + pool + relu)
    y, dzp = a["y"], a["dz"]
    fw, rh = host_model(O, a, relu, pool, dzp)
    base = dict(y=y, gamma=a["gamma"], beta=a["beta"])
    outs = dict(sm=c, si=c, z=(groups, c), ties=(groups, c))
    runs = [call(raw, dev, FWD, base, outs, rows=rows, c=c, relu=relu, pool=pool)]
    for mode in (0, 1):
        runs.append(call(raw, dev, FWD_POOL, base, dict(outs, ysel=(groups, c)), rows=rows, c=c, relu=relu, pool=pool, mode=mode))
    memo = {}

    def restated(r):    # the forward restated from a run's own saved moments (the three runs nearly always save the same bits)
        key = r["sm"].tobytes() + r["si"].tobytes()
        if key not in memo:
            memo[key] = B.restate(y, a["gamma"], a["beta"], relu, r["sm"], r["si"], pool=pool)
        return memo[key]
    for r in runs:
        nt.ulp("save_mean", r["sm"], fw["mean"])
        nt.ulp("save_invstd", r["si"], fw["invstd"])
        nt.within("zmax", r["z"], fw["zmax"], rh["zmax"])
        rk = restated(r)
        assert same_bits(r["z"], rk["zmax"]), "zmax differs from the restatement from the saved moments"
        assert same_bits(r["ties"], rk["ties"]), "ties differ"
        assert "ysel" not in r or same_bits(r["ysel"], rk["ysel"]), "ysel is not the y of the first row attaining the maximum"
    assert (rk["ties"][1] == pool).all() and (rk["ties"][::3, 2] == pool - pool // 2 + 1).all()     # identical rows; repeated rows
    assert (rk["ties"][:, 1] == pool).all() and bool(np.signbit(rk["zmax"][0, 1])) == (not relu)      # +-0: all rows tie
    assert not relu or ((rk["ties"][:, 0] == pool).all() and not rk["zmax"][:, 0].any())             # dead channel: ties at 0
    if reduction_blocks(rows, c) == 1:
        assert all(same_bits(r["z"], runs[0]["z"]) and same_bits(r["ties"], runs[0]["ties"]) for r in runs[1:])
    # backward from the pooled entry point's outputs; the float64 reference takes the kernel's tie pattern and ReLU mask
    p = runs[1]
    rk = restated(p)
    ref = B.backward64(O, y, a["gamma"], a["beta"], dzp, relu, EPS, pool, z_pattern=rk["z"])
    bin_ = dict(base, dz=dzp, sm=p["sm"], si=p["si"], zmax=p["z"], ties=p["ties"])
    bout = dict(dy=(rows, c), dgamma=c, dbeta=c)
    check_backward(nt, call(raw, dev, BWD, bin_, bout, rows=rows, c=c, relu=relu, pool=pool), ref, rh, rows)
    check_backward(nt, call(raw, dev, BWD_MODE, bin_, bout, rows=rows, c=c, relu=relu, pool=pool, mode=1), ref, rh, rows)
    gout = dict(coef=(6, c), dgamma=c, dbeta=c)
    g = call(raw, dev, GCONST, bin_, gout, rows=rows, c=c, relu=relu, pool=pool, stats_done=0)
    check_coef_head(g, a, p["sm"], p["si"])
    check_backward(nt, g, ref, rh, rows, coef_only=True)
    g = call(raw, dev, GCONST, dict(bin_, ysel=p["ysel"]), gout, rows=rows, c=c, relu=relu, pool=pool, stats_done=0)
    check_coef_head(g, a, p["sm"], p["si"])
    check_backward(nt, g, ref, rh, rows, coef_only=True, pooled=True)
    # channel 1 of the pooled reduction against the same float64 sum of the same float32 terms, from the kernel's saved moments
    # and the (verified) ysel: another order of an fp64 sum moves it by groups * 2^-53 of sum |terms|, the rounding to float32 by
    # half an ulp of the result -- together below 1 float32 ulp of sum |terms|
    with np.errstate(all="ignore"):
        gd = np.where((p["z"][:, 1] > 0) | (not relu), dzp[:, 1], np.float32(0)).astype(np.float64)
        terms = gd * B.xhat32(p["ysel"][:, 1], p["sm"][1], p["si"][1]).astype(np.float64)
    tol = float(B.ulp32(np.abs(terms).sum()))
    assert abs(float(g["dgamma"][1]) - terms.sum()) <= tol, "pooled dgamma of the +-0 channel: %r vs %r" % (g["dgamma"][1], terms.sum())
    assert abs(float(g["coef"][5][1]) - terms.sum() / rows) <= tol / rows, "pooled k2 of the +-0 channel"
    assert abs(float(g["dbeta"][1]) - gd.sum()) <= float(B.ulp32(np.abs(gd).sum()))


@pytest.mark.parametrize("pool", [2, 3, 7, 8, 9, 15, 17, 33])
@pytest.mark.parametrize("c", [5, 36, 1020])
def test_pool_sweep(pn2, oracle, cuda, c, pool):
    """pool in {2, 3, 7, 8, 9, 15, 17, 33} (below 8, not a multiple of 8: the tail of the 8-rows-in-flight loop) x c in
    {5, 36, 1020} x relu in {0, 1}, 67 groups, plus the largest group count that still fits one reduction block: pn2_bn_relu_forward
    (pool) and pn2_bn_relu_forward_pool in stats modes 0 and 1 -- zmax, ties, ysel bit-equal to the restatement from the saved
    moments (duplicated rows, a group of identical rows, dead channels tying at the ReLU floor with different y, +-0), the entry
    points bit-equal to each other at one-block shapes; pn2_bn_relu_backward (pool), pn2_bn_relu_backward_mode (1) and
    pn2_bn_grad_constants without and with ysel within the measured bound (the pooled reduction against its own restatement:
    dzp instead of n * fl(dzp / n), xh of ysel).  Channel 1 without ReLU, where rows of different y tie and the pooled form
    stands for all of them by the first, is outside what that form represents (its restatement is 6e8 ulp from float64): there
    the kernel's pooled dgamma / k2 / dbeta are held to the float64 sum of the same float32 terms within 1 ulp of sum |terms|.

    Measured restatement error, worst over the sweep, in ulps of the output scale: zmax 16, dy 11, dgamma 12 (pooled form 12),
    dbeta 1.0 (pooled 0.5), k1 1.2 (0.5), k2 13 (13) -- the large figures at the 2- and 4-group shapes."""
    raw = pn2._lib._raw
    nt = Notes("pool c=%d pool=%d" % (c, pool))
    small = 8 * mapping(c)[2] // pool
    for relu in (0, 1):
        check_pool(raw, oracle, cuda, 67, pool, c, relu, nt)
        if small >= 2:
            assert reduction_blocks(small * pool, c) == 1
            check_pool(raw, oracle, cuda, small, pool, c, relu, nt)
    nt.done()


@pytest.mark.parametrize("c", [1020, 255])
def test_pool_grid_stride(pn2, oracle, cuda, c):
    """bn_apply_pool_kernel's grid is capped at 2048 blocks of rp groups: with rp = 1 (c = 1020 on the 16-byte path, c = 255 on
    the scalar one) 2048 + 5 groups of 2 rows make five blocks take a second pass.  Same checks as test_pool_sweep.

    Measured restatement error in ulps of the output scale: zmax 1.3, dy 1.8, dgamma 1.3, dbeta 0.5, k1 0.5, k2 1.3 (the pooled
    form the same)."""
    assert mapping(c)[2] == 1
    nt = Notes("pool grid-stride c=%d" % c)
    for relu in (0, 1):
        check_pool(pn2._lib._raw, oracle, cuda, 2048 + 5, 2, c, relu, nt)
    nt.done()


# ==================================================================================================== 3. numerics
def test_cancellation_needs_float64_sums(pn2, oracle, cuda):
    """5000 rows of 64 + 0.05 * randn (E[y^2] ~ 4096, var ~ 0.0025, eps = 1e-3): save_invstd of pn2_bn_relu_forward and of the
    deferred form within 2 ulp of the exact two-pass value.  tests/test_bn_edges_cpu.py shows that float64 sums meet this in any
    order (0.054 ulp before the final rounding) and float32 sums miss it by 2.9e6 ulp."""
    raw = pn2._lib._raw
    y = B.cancellation_input()
    rows, c = y.shape
    exact = np.array([B.moments_two_pass(y[:, ch]) for ch in range(c)])
    inv = 1.0 / np.sqrt(exact[:, 1] + EPS)
    base = dict(y=y, gamma=np.ones(c, np.float32), beta=np.zeros(c, np.float32))
    nt = Notes("cancellation")
    f = call(raw, cuda, FWD, base, dict(sm=c, si=c, z=(rows, c)), rows=rows, c=c, relu=0, pool=0)
    d = call(raw, cuda, FWD_DEF, base, dict(sm=c, si=c, scale=c, shift=c), rows=rows, c=c, stats_done=0)
    for r in (f, d):
        nt.ulp("save_invstd", r["si"], inv, 2.0)
        nt.ulp("save_mean", r["sm"], exact[:, 0])
    nt.done()


def numerics_case(raw, O, dev, a, nt, relu=1):
    """forward + backward + gradient constants of one input against float64 -> (forward, backward, constants) results"""
    rows, c = a["y"].shape
    fw, rh = host_model(O, a, relu, dz=a["dz"])
    base = dict(y=a["y"], gamma=a["gamma"], beta=a["beta"])
    f = call(raw, dev, FWD, base, dict(sm=c, si=c, z=(rows, c)), rows=rows, c=c, relu=relu, pool=0)
    nt.ulp("save_mean", f["sm"], fw["mean"])
    nt.ulp("save_invstd", f["si"], fw["invstd"])
    nt.within("z", f["z"], fw["z"], rh["z"])
    ref = B.backward64(O, a["y"], a["gamma"], a["beta"], a["dz"], relu, EPS, 0, z_pattern=f["z"])
    bin_ = dict(base, dz=a["dz"], sm=f["sm"], si=f["si"])
    b = call(raw, dev, BWD, bin_, dict(dy=(rows, c), dgamma=c, dbeta=c), rows=rows, c=c, relu=relu, pool=0)
    nt.within("dy", b["dy"], ref[0], rh["dy"], own=rh["dy64"])
    nt.within("dgamma", b["dgamma"], ref[1], rh["dgamma"], own=rh["dg64"])
    nt.within("dbeta", b["dbeta"], ref[2], rh["dbeta"], own=rh["db64"])
    return fw, f, b


def test_constant_channels(pn2, oracle, cuda):
    """every row holds the same value (0, +-3.7, 100, 64, 1e-20, ... per channel; |y| <= 100 because the one-pass variance in
    float64 is only exact to a few 2^-53 * mean^2 = 4e-12 there, 4e-9 of eps, far below a float32 ulp of invstd):
    invstd = float32(1 / sqrt(eps)) within 1 ulp, z within the measured bound of beta (the restatement's own error grows with
    |y| * sc: sh = fl(beta - mean * sc) is rounded at that size), dy finite and within bound.  Measured restatement error in ulps of the output scale: z 2.0e3 (the
    channel of 100), dy 0.77, dbeta 0.24."""
    rows, c = 300, 8
    a = plain_input(rows, c, 5)
    a["y"] = np.tile(np.array([0.0, 3.7, -3.7, 100.0, -0.001, 64.0, 1e-20, 7.0], np.float32), (rows, 1))
    nt = Notes("constant channels")
    fw, f, b = numerics_case(pn2._lib._raw, oracle, cuda, a, nt, relu=0)
    nt.ulp("save_invstd", f["si"], np.full(c, 1.0 / np.sqrt(EPS)))
    assert np.abs(fw["z"] - a["beta"].astype(np.float64)).max() < 1e-9 and np.isfinite(b["dy"]).all()
    nt.done()


def test_large_magnitude_channel(pn2, oracle, cuda):
    """one channel of +-1e30 (its squares overflow float32, its fp64 sums do not): finite results, saved moments within 1 ulp,
    z / dy / dgamma / dbeta within the measured bound taken per channel, dy of that channel (of size 1e-30) also on its own
    scale.  Measured restatement error in ulps of the output scale: z 0.92, dy 0.69 (that channel alone 0.76), dgamma 2.7,
    dbeta 0.34."""
    rows, c = 1000, 8
    a = plain_input(rows, c, 6)
    rs = np.random.RandomState(60)
    a["y"][:, 3] = (np.where(rs.rand(rows) < 0.5, -1.0, 1.0) * 1e30 * (1.0 + 0.1 * rs.randn(rows))).astype(np.float32)
    nt = Notes("large magnitude")
    fw, f, b = numerics_case(pn2._lib._raw, oracle, cuda, a, nt, relu=1)
    for r in (f["sm"], f["si"], f["z"], b["dy"], b["dgamma"], b["dbeta"]):
        assert np.isfinite(r).all()
    _, rh = host_model(oracle, a, 1, dz=a["dz"])
    ref = B.backward64(oracle, a["y"], a["gamma"], a["beta"], a["dz"], 1, EPS, 0, z_pattern=f["z"])
    nt.within("dy[1e30 channel]", b["dy"][:, 3], ref[0][:, 3], rh["dy"][:, 3], per_channel=False, own=rh["dy64"][:, 3])   # on its own scale (1e-30)
    assert fw["var"][3] > 1e59
    nt.done()


@pytest.mark.parametrize("c", [12, 7])
def test_channel_isolation(pn2, oracle, cuda, c):
    """NaN in one channel, +inf in a second, +-1e30 in a third: at a one-reduction-block shape every OTHER channel's outputs --
    forward, backward, deferred constants, gradient constants, moving averages -- are bit-identical to a run in which those three
    channels hold ordinary numbers; at a 34-block shape (atomics in another order) they stay within the measured bound."""
    raw = pn2._lib._raw
    rp = mapping(c)[2]
    bad = [2, 4, 6] if c == 7 else [2, 5, 9]
    good = [ch for ch in range(c) if ch not in bad]
    nt = Notes("isolation c=%d" % c)
    for rows in (8 * rp, 33 * 8 * rp + 3):
        a = plain_input(rows, c, 9 * c + rows)
        dirty = dict(a, y=a["y"].copy())
        dirty["y"][::3, bad[0]] = np.nan
        dirty["y"][1::4, bad[1]] = np.inf
        dirty["y"][:, bad[2]] = np.where(np.arange(rows) % 2, -1e30, 1e30).astype(np.float32)
        fw, rh = host_model(oracle, a, 1, dz=a["dz"])
        rm0, rv0 = np.full(c, 0.25, np.float32), np.full(c, 2.0, np.float32)
        res = []
        for case in (a, dirty):
            base = dict(y=case["y"], gamma=a["gamma"], beta=a["beta"])
            f = call(raw, cuda, FWD, dict(base, bias=a["bias"], rm=rm0, rv=rv0), dict(sm=c, si=c, z=(rows, c)), rows=rows, c=c, relu=1, pool=0)
            bin_ = dict(base, dz=a["dz"], sm=f["sm"], si=f["si"])
            b = call(raw, cuda, BWD, bin_, dict(dy=(rows, c), dgamma=c, dbeta=c), rows=rows, c=c, relu=1, pool=0)
            d = call(raw, cuda, FWD_DEF, dict(base, rm=rm0, rv=rv0), dict(sm=c, si=c, scale=c, shift=c), rows=rows, c=c, stats_done=0)
            g = call(raw, cuda, GCONST, bin_, dict(coef=(6, c), dgamma=c, dbeta=c), rows=rows, c=c, relu=1, pool=0, stats_done=0)
            res.append(dict(sm=f["sm"], si=f["si"], z=f["z"], rm=f["rm"], rv=f["rv"], dy=b["dy"], dgamma=b["dgamma"], dbeta=b["dbeta"],
                            dsm=d["sm"], dsi=d["si"], scale=d["scale"], shift=d["shift"], drm=d["rm"], drv=d["rv"], coef=g["coef"],
                            gdgamma=g["dgamma"], gdbeta=g["dbeta"]))
        clean, got = res
        if reduction_blocks(rows, c) == 1:
            for k in clean:
                assert same_bits(clean[k][..., good], got[k][..., good]), "%s of the other channels changed (c=%d rows=%d)" % (k, c, rows)
        ref = B.backward64(oracle, a["y"], a["gamma"], a["beta"], a["dz"], 1, EPS, 0, z_pattern=np.where(np.isfinite(got["z"]), got["z"], 0))
        nt.ulp("save_mean", got["sm"][good], fw["mean"][good])
        nt.ulp("save_invstd", got["si"][good], fw["invstd"][good])
        nt.within("z", got["z"][:, good], fw["z"][:, good], rh["z"][:, good])
        nt.within("dy", got["dy"][:, good], ref[0][:, good], rh["dy"][:, good], own=rh["dy64"][:, good])
        for k, i, h, o in (("dgamma", 1, "dgamma", "dg64"), ("dbeta", 2, "dbeta", "db64"), ("gdgamma", 1, "dgamma", "dg64"),
                           ("gdbeta", 2, "dbeta", "db64")):
            nt.within(k, got[k][good], ref[i][good], rh[h][good], own=rh[o][good])
        nt.within("k1", got["coef"][4][good], ref[2][good] / rows, rh["k1"][good], own=rh["db64"][good] / rows)
        nt.within("k2", got["coef"][5][good], ref[1][good] / rows, rh["k2"][good], own=rh["dg64"][good] / rows)
    nt.done()


# =================================================================================================== 4. workspace
@pytest.mark.parametrize("c", [5, 36])
def test_mode_0_on_a_dirty_workspace(pn2, oracle, cuda, c):
    """the entry points that zero the workspace themselves (pn2_bn_relu_forward, pn2_bn_relu_backward, _forward_mode (0),
    _backward_mode (0), _forward_pool (0)) on a workspace pre-filled with 0xFF bytes: bit-equal to a run on a zeroed one at a
    one-block shape, within the measured bound at a 34-block shape (head, folded sums and both slot copies must be cleared)."""
    raw = pn2._lib._raw
    rp = mapping(c)[2]
    nt = Notes("dirty workspace c=%d" % c)
    for rows in (8 * rp, 33 * 8 * rp + 2):
        assert reduction_blocks(rows, c) == (1 if rows == 8 * rp else 34) and rows % 2 == 0
        a = plain_input(rows, c, 13 * c + rows)
        dzp = a["dz"][:rows // 2]
        fw, rh = host_model(oracle, a, 1, dz=a["dz"])
        fwp, rhp = host_model(oracle, a, 1, 2, dzp)
        base = dict(y=a["y"], gamma=a["gamma"], beta=a["beta"])
        out = {}
        for fill in (0, 0xFF):
            o = out.setdefault(fill, {})
            fo = dict(sm=c, si=c, z=(rows, c))
            o["fwd"] = call(raw, cuda, FWD, base, fo, ws_fill=fill, rows=rows, c=c, relu=1, pool=0)
            o["fwd_mode"] = call(raw, cuda, FWD_MODE, base, fo, ws_fill=fill, rows=rows, c=c, relu=1, mode=0)
            o["fwd_pool"] = call(raw, cuda, FWD_POOL, base, dict(sm=c, si=c, z=(rows // 2, c), ties=(rows // 2, c), ysel=(rows // 2, c)),
                                 ws_fill=fill, rows=rows, c=c, relu=1, pool=2, mode=0)
            f, p = out[0]["fwd"], out[0]["fwd_pool"]
            bin_ = dict(base, dz=a["dz"], sm=f["sm"], si=f["si"])
            bo = dict(dy=(rows, c), dgamma=c, dbeta=c)
            o["bwd"] = call(raw, cuda, BWD, bin_, bo, ws_fill=fill, rows=rows, c=c, relu=1, pool=0)
            o["bwd_mode"] = call(raw, cuda, BWD_MODE, bin_, bo, ws_fill=fill, rows=rows, c=c, relu=1, pool=0, mode=0)
            o["bwd_pool"] = call(raw, cuda, BWD, dict(base, dz=dzp, sm=p["sm"], si=p["si"], zmax=p["z"], ties=p["ties"]), bo, ws_fill=fill,
                                 rows=rows, c=c, relu=1, pool=2)
        for k, r in out[0xFF].items():
            names = [n for n in r if not n.startswith("_")]
            if reduction_blocks(rows, c) == 1:
                assert all(same_bits(r[n], out[0][k][n]) for n in names), "%s differs on a dirty workspace" % k
            if "sm" in r:
                nt.ulp("save_mean", r["sm"], fw["mean"])
                nt.ulp("save_invstd", r["si"], fw["invstd"])
        for k in ("fwd", "fwd_mode"):
            nt.within("z", out[0xFF][k]["z"], fw["z"], rh["z"])
        nt.within("zmax", out[0xFF]["fwd_pool"]["z"], fwp["zmax"], rhp["zmax"])
        ref = B.backward64(oracle, a["y"], a["gamma"], a["beta"], a["dz"], 1, EPS, 0, z_pattern=out[0]["fwd"]["z"])
        for k in ("bwd", "bwd_mode"):
            check_backward(nt, out[0xFF][k], ref, rh, rows)
        p = out[0]["fwd_pool"]
        rk = B.restate(a["y"], a["gamma"], a["beta"], 1, p["sm"], p["si"], pool=2)
        check_backward(nt, out[0xFF]["bwd_pool"], B.backward64(oracle, a["y"], a["gamma"], a["beta"], dzp, 1, EPS, 2, z_pattern=rk["z"]), rhp, rows)
    nt.done()


@pytest.mark.parametrize("rows,cout", [(40, 32), (40, 96), (1000, 32), (1000, 96)])
def test_stats_modes_2_and_3_after_the_gemm_producers(pn2, oracle, cuda, rows, cout):
    """y and its column sums from pn2_linear_bn_stats (mode 2: sums in all slot copies, not folded) and pn2_linear_bn_stats_fin
    with finish = 1 (mode 3: folded), cin = 8: pn2_bn_relu_forward_mode and pn2_bn_relu_forward_pool (pool 8) in those modes
    against the float64 batch norm of the y read back from the device -- saved moments within 1 ulp, z within the measured
    bound, zmax / ties / ysel bit-equal to the restatement from the saved moments."""
    import torch
    raw = pn2._lib._raw
    cin, pool = 8, 8
    rs = np.random.RandomState(rows + cout)
    a = plain_input(rows, cout, rows * 3 + cout)
    x, w = Buf(cuda, (rows, cin), rs.randn(rows, cin)), Buf(cuda, (cin, cout), rs.randn(cin, cout) * 0.5 + 0.2)
    nt = Notes("stats modes rows=%d cout=%d" % (rows, cout))
    for mode in (2, 3):
        ws, by = Ws(raw, cuda, cout, 0), Buf(cuda, (rows, cout))
        if mode == 2:
            rc = raw.pn2_linear_bn_stats(rows, cin, cout, x.ptr(), w.ptr(), by.ptr(), ws.ptr(), ws.nbytes, None)
        else:
            rc = raw.pn2_linear_bn_stats_fin(rows, cin, cout, x.ptr(), w.ptr(), by.ptr(), ws.ptr(), ws.nbytes, None, None, 0, 1, None, None,
                                             None, EPS, DECAY, None, None, None, None, None, None, None)
        torch.cuda.synchronize()
        assert rc == 0
        ws.raw()
        y = by.get()
        by.init = y.reshape(-1)          # from here on an input: must stay as the GEMM wrote it
        case = dict(y=y, gamma=a["gamma"], beta=a["beta"])
        fw, rh = host_model(oracle, case, 1)
        fwp, rhp = host_model(oracle, case, 1, pool)
        base = dict(case, y=by)
        f = call(raw, cuda, FWD_MODE, base, dict(sm=cout, si=cout, z=(rows, cout)), ws=ws, rows=rows, c=cout, relu=1, mode=mode)
        p = call(raw, cuda, FWD_POOL, base, dict(sm=cout, si=cout, z=(rows // pool, cout), ties=(rows // pool, cout), ysel=(rows // pool, cout)),
                 ws=ws, rows=rows, c=cout, relu=1, pool=pool, mode=mode)
        for r in (f, p):
            nt.ulp("save_mean", r["sm"], fw["mean"])
            nt.ulp("save_invstd", r["si"], fw["invstd"])
        nt.within("z", f["z"], fw["z"], rh["z"])
        nt.within("zmax", p["z"], fwp["zmax"], rhp["zmax"])
        rk = B.restate(y, a["gamma"], a["beta"], 1, p["sm"], p["si"], pool=pool)
        assert same_bits(p["z"], rk["zmax"]) and same_bits(p["ties"], rk["ties"]) and same_bits(p["ysel"], rk["ysel"])
    nt.done()


# ========================================================================================== 5. misaligned operands
def test_misaligned_operands_take_the_scalar_path(pn2, oracle, cuda):
    """c % 4 == 0 and c <= 256 with y, z, dz or dy (each in turn) 4 bytes off a 16-byte boundary: the call succeeds on the scalar
    path, results within the measured bound, margins intact."""
    raw = pn2._lib._raw
    rows, c = 300, 36
    a = plain_input(rows, c, 3)
    fw, rh = host_model(oracle, a, 1, dz=a["dz"])
    base = dict(y=a["y"], gamma=a["gamma"], beta=a["beta"])
    nt = Notes("misaligned c=%d" % c)
    for off in ("y", "z"):
        f = call(raw, cuda, FWD, base, dict(sm=c, si=c, z=(rows, c)), off=(off,), rows=rows, c=c, relu=1, pool=0)
        nt.ulp("save_mean", f["sm"], fw["mean"])
        nt.ulp("save_invstd", f["si"], fw["invstd"])
        nt.within("z", f["z"], fw["z"], rh["z"])
    ref = B.backward64(oracle, a["y"], a["gamma"], a["beta"], a["dz"], 1, EPS, 0, z_pattern=f["z"])
    for off in ("dz", "dy", "y"):
        b = call(raw, cuda, BWD, dict(base, dz=a["dz"], sm=f["sm"], si=f["si"]), dict(dy=(rows, c), dgamma=c, dbeta=c), off=(off,),
                 rows=rows, c=c, relu=1, pool=0)
        check_backward(nt, b, ref, rh, rows)
    nt.done()


def test_misaligned_operands_are_refused_where_the_scalar_path_ends(pn2, cuda):
    """c = 260 (more than 256 scalar columns) with a misaligned operand: PN2_EUNSUP from every entry point, all outputs and the
    workspace bit-unchanged.  A misaligned zmax / ties (pooled backward, pn2_bn_grad_constants) or ysel (pn2_bn_relu_forward_pool)
    next to aligned 16-byte operands: PN2_EINVAL."""
    raw = pn2._lib._raw
    rows, c = 40, 260
    a = plain_input(rows, c, 4)
    base = dict(y=a["y"], gamma=a["gamma"], beta=a["beta"])
    v = np.ones(c, np.float32)
    fo, bo, go = dict(sm=c, si=c, z=(rows, c)), dict(dy=(rows, c), dgamma=c, dbeta=c), dict(coef=(6, c), dgamma=c, dbeta=c)
    bin_ = dict(base, dz=a["dz"], sm=v, si=v)
    rm = dict(rm=v, rv=v)
    for off in ("y", "z"):
        call(raw, cuda, FWD, dict(base, **rm), fo, off=(off,), expect=EUNSUP, ws_fill=0xFF, rows=rows, c=c, relu=1, pool=0)
        call(raw, cuda, FWD_MODE, dict(base, **rm), fo, off=(off,), expect=EUNSUP, ws_fill=0xFF, rows=rows, c=c, relu=1, mode=0)
    call(raw, cuda, FWD_DEF, dict(base, **rm), dict(sm=c, si=c, scale=c, shift=c), off=("y",), expect=EUNSUP, rows=rows, c=c, stats_done=0)
    for off in ("dz", "dy", "y"):
        call(raw, cuda, BWD, bin_, bo, off=(off,), expect=EUNSUP, ws_fill=0xFF, rows=rows, c=c, relu=1, pool=0)
    for off in ("dz", "y"):
        call(raw, cuda, GCONST, bin_, go, off=(off,), expect=EUNSUP, rows=rows, c=c, relu=1, pool=0, stats_done=0)
    pz = dict(z=(rows // 2, c), ties=(rows // 2, c), ysel=(rows // 2, c))
    call(raw, cuda, FWD_POOL, base, dict(sm=c, si=c, **pz), off=("ties",), expect=EUNSUP, rows=rows, c=c, relu=1, pool=2, mode=0)
    for cc in (36, 260):
        a = plain_input(rows, cc, 5)
        base = dict(y=a["y"], gamma=a["gamma"], beta=a["beta"])
        v = np.ones(cc, np.float32)
        half = np.ones((rows // 2, cc), np.float32)
        pin = dict(base, dz=half, sm=v, si=v, zmax=half, ties=half)
        for off in ("zmax", "ties"):
            call(raw, cuda, BWD, pin, dict(dy=(rows, cc), dgamma=cc, dbeta=cc), off=(off,), expect=EINVAL, ws_fill=0xFF, rows=rows, c=cc,
                 relu=1, pool=2)
            call(raw, cuda, BWD_MODE, pin, dict(dy=(rows, cc), dgamma=cc, dbeta=cc), off=(off,), expect=EINVAL, ws_fill=0xFF, rows=rows, c=cc,
                 relu=1, pool=2, mode=1)
            for ysel in (None, half):
                call(raw, cuda, GCONST, dict(pin, ysel=ysel), dict(coef=(6, cc), dgamma=cc, dbeta=cc), off=(off,), expect=EINVAL, rows=rows,
                     c=cc, relu=1, pool=2, stats_done=0)
        call(raw, cuda, FWD_POOL, base, dict(sm=cc, si=cc, z=(rows // 2, cc), ties=(rows // 2, cc), ysel=(rows // 2, cc)), off=("ysel",),
             expect=EINVAL, ws_fill=0xFF, rows=rows, c=cc, relu=1, pool=2, mode=0)


# ============================================================================================ 6. argument contracts
def test_argument_contracts(pn2, cuda):
    """What the existing argument test does not assert: pn2_bn_relu_forward_pool (pool <= 1, stats_mode outside [0, 3]:
    PN2_EINVAL; NULL ysel: PN2_ENULL), _forward_mode / _backward_mode (stats_mode outside [0, 3]), the backward (pool > 1 with
    dy == dz, mode >= 2 with pool > 1, rows % pool != 0: PN2_EINVAL; each NULL pointer: PN2_ENULL) and pn2_bn_grad_constants
    (stats_done with pool > 1: PN2_EINVAL; NULL pointers).  In every case no output, moving average or workspace word changes
    (the workspace holds 0xFF bytes: a memset before the refusal would show)."""
    raw = pn2._lib._raw
    rows, c = 16, 8
    a = plain_input(rows, c, 8)
    v = np.ones(c, np.float32)
    half = np.ones((rows // 2, c), np.float32)
    base = dict(y=a["y"], gamma=a["gamma"], beta=a["beta"], rm=v, rv=v)
    po = dict(sm=c, si=c, z=(rows // 2, c), ties=(rows // 2, c), ysel=(rows // 2, c))
    kw = dict(rows=rows, c=c, relu=1, ws_fill=0xFF)
    for pool in (1, 0, -3):
        call(raw, cuda, FWD_POOL, base, po, expect=EINVAL, pool=pool, mode=0, **kw)
    for mode in (-1, 4):
        call(raw, cuda, FWD_POOL, base, po, expect=EINVAL, pool=2, mode=mode, **kw)
        call(raw, cuda, FWD_MODE, base, dict(sm=c, si=c, z=(rows, c)), expect=EINVAL, mode=mode, **kw)
    call(raw, cuda, FWD_POOL, base, po, null=("ysel",), expect=ENULL, pool=2, mode=0, **kw)
    call(raw, cuda, FWD_POOL, base, po, expect=EINVAL, pool=3, mode=0, **kw)                      # 16 rows, groups of 3
    bin_ = dict(y=a["y"], gamma=a["gamma"], beta=a["beta"], dz=a["dz"], sm=v, si=v)
    pin = dict(bin_, dz=half, zmax=half, ties=half)
    bo, go = dict(dy=(rows, c), dgamma=c, dbeta=c), dict(coef=(6, c), dgamma=c, dbeta=c)
    for mode in (-1, 4):
        call(raw, cuda, BWD_MODE, bin_, bo, expect=EINVAL, pool=0, mode=mode, **kw)
    call(raw, cuda, BWD, dict(pin, dz=a["dz"]), bo, alias={"dy": "dz"}, expect=EINVAL, pool=2, **kw)    # pooled, in place
    for mode in (2, 3):
        call(raw, cuda, BWD_MODE, pin, bo, expect=EINVAL, pool=2, mode=mode, **kw)
    call(raw, cuda, BWD, pin, bo, expect=EINVAL, pool=3, **kw)
    call(raw, cuda, GCONST, pin, go, expect=EINVAL, pool=3, stats_done=0, **kw)
    for ysel in (None, half):
        call(raw, cuda, GCONST, dict(pin, ysel=ysel), go, expect=EINVAL, pool=2, stats_done=1, **kw)
    for name in ("dz", "y", "gamma", "beta", "sm", "si", "ws", "dy", "dgamma", "dbeta"):
        call(raw, cuda, BWD, bin_, bo, null=(name,), expect=ENULL, pool=0, **kw)
        call(raw, cuda, BWD_MODE, bin_, bo, null=(name,), expect=ENULL, pool=0, mode=1, **kw)
    for name in ("dz", "y", "gamma", "beta", "sm", "si", "ws", "coef", "dgamma", "dbeta"):
        call(raw, cuda, GCONST, bin_, go, null=(name,), expect=ENULL, pool=0, stats_done=0, **kw)
    for name in ("zmax", "ties"):
        call(raw, cuda, BWD, pin, bo, null=(name,), expect=ENULL, pool=2, **kw)
        call(raw, cuda, GCONST, pin, go, null=(name,), expect=ENULL, pool=2, stats_done=0, **kw)
    for name in ("y", "gamma", "beta", "ws", "sm", "si", "z", "ties"):
        call(raw, cuda, FWD_POOL, base, po, null=(name,), expect=ENULL, pool=2, mode=0, **kw)
    for name in ("y", "gamma", "beta", "ws", "sm", "si", "scale", "shift", "rm", "rv"):
        call(raw, cuda, FWD_DEF, base, dict(sm=c, si=c, scale=c, shift=c), null=(name,), expect=ENULL, rows=rows, c=c, stats_done=0, ws_fill=0xFF)
