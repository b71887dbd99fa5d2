"""Every kernel call of a real training step -- at the full semantic size (B=16, N=8192, npoint 1024/256/64/16: the only shape
at which the streaming kernels of the training GEMMs run inside the model) and at the small size of the other whole-model tests
-- checked as it happens against float64 of its OWN operands.  The chain of 23 batch norms makes whole-model comparisons loose
(tests/test_layers_gpu.py::test_training_gradients_with_hip_wgrad_match_torch); call by call it does not matter."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, s_scene
from test_layers_gpu import T

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24  # unit roundoff of float32
# the entry points of the dense layers' kernels; every launch of one of these in the audited step must lie inside an audited call
GEMM_LAUNCHES = frozenset({"pn2_linear", "pn2_linear_narrow", "pn2_linear_bn_stats", "pn2_linear_bn_stats_xf", "pn2_linear_bn_stats_fin",
                           "pn2_linear_dgrad", "pn2_linear_dgrad_bn_grad_stats", "pn2_linear_dgrad_gx", "pn2_linear_dgrad_fin",
                           "pn2_linear_bwd_fused", "pn2_linear_wgrad", "pn2_linear_wgrad_accumulate", "pn2_linear_wgrad_accumulate_xf",
                           "pn2_linear_wgrad_gx", "pn2_bn_grad_constants"})
FWD_LAUNCHES = ("pn2_linear_bn_stats", "pn2_linear_bn_stats_xf", "pn2_linear_bn_stats_fin")
WGRAD_LAUNCHES = ("pn2_linear_wgrad", "pn2_linear_wgrad_accumulate", "pn2_linear_wgrad_accumulate_xf", "pn2_linear_wgrad_gx")


def stream_min_rows():
    """PN2_STREAM_MIN_ROWS as the library was built with it (csrc/pn2_common.h)"""
    with open(os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd", "csrc", "pn2_common.h")) as f:
        return int(re.search(r"#define\s+PN2_STREAM_MIN_ROWS\s+(\d+)", f.read()).group(1))


def _aligned(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


# Python restatements of the three gates (csrc/pn2_fwd_narrow.h fwd_narrow_fits, csrc/pn2_dgrad_wide.h dgrad_wide_fits, the
# eight-wave tile of linear_wgrad_impl in csrc/pn2_linear.hip)
def fwd_narrow_fits(rows, cin, cout, min_rows):
    if cin not in (32, 64) and not (cin == 128 and cout == 128):
        return False
    return cout in (32, 64, 128) and rows % 32 == 0 and rows >= min_rows


def dgrad_wide_fits(rows, n_in, n_out, pool, min_rows):
    return n_out == 128 and n_in in (64, 128) and pool in (0, 32) and rows % 32 == 0 and rows >= min_rows


def wide8(rows, cin, cout, min_rows):
    return cin > 32 and cout > 64 and rows >= min_rows


def fwd_stream_workgroups(rows, cin):
    """workgroups of the streaming forward launch (launch_fwd_narrow_one / fwd_wide_in)"""
    return min((rows // 32 + 7) // 8, 256) if cin == 128 else min((rows // 32 + 3) // 4, 1024)


def dgrad_wide_workgroups(rows):
    return min((rows // 32 + 7) // 8, 256)


def _batch(cuda, b, n, seed=0):
    """tests/test_train_gpu.py::_batch at any size: xyz of an S-scene + rgb, labels, weights"""
    rs = np.random.RandomState(seed)
    pc = T(np.concatenate([s_scene(seed + 1, b, n), rs.random_sample((b, n, 3)).astype(np.float32)], 2), cuda)
    labels = T(rs.randint(0, 9, (b, n)).astype(np.int64), cuda)
    smpw = T((rs.random_sample((b, n)) + 0.5).astype(np.float32), cuda)
    return pc, labels, smpw


def _rel(got, ref):
    return float((got.double() - ref).norm() / max(float(ref.norm()), 1e-300))


def _fma(x, sc, sh, relu):
    """relu?(fmaf(x, sc, sh)): one rounding of the exact value, as the kernels form an operand on load"""
    a = (x.double() * sc.double() + sh.double()).float()
    return a.clamp_min(0.0) if relu else a


def _bn_affine(gamma, beta, mean, invstd):
    """bn_scale_shift (csrc/pn2_common.h): sc = gamma * invstd, sh = fmaf(-mean, sc, beta), in float32"""
    sc = gamma * invstd
    return sc, (-mean.double() * sc.double() + beta.double()).float()


def dy_on_load(y, dz, coef, relu, pool, zmax, ties):
    """the gradient leaving a batch norm (+ReLU, + max over `pool` rows) as the kernels form it while loading (y, dz)
    (tests/test_train_gpu.py::test_every_gemm_of_a_real_step_is_as_accurate_as_the_library) -> dy, g * mask"""
    sc, sh, mu, is_, k1, k2 = coef
    lin = y.double() * sc.double() + sh.double()
    on = (lin > 0) if relu else torch.ones_like(lin, dtype=torch.bool)
    del lin
    if pool:
        ties = ties[0] if ties.dim() == zmax.dim() + 1 else ties  # [tie counts | ysel] of the pooled forward
        t = torch.where(on, y.double() * sc.double() + sh.double(), 0.0).float().view(-1, pool, y.shape[1])
        g = torch.where(t == zmax.view(-1, 1, y.shape[1]), (dz / ties).view(-1, 1, y.shape[1]), 0.0).view_as(y)
    else:
        g = dz
    gk = torch.where(on, g, 0.0)
    return sc * (-((y - mu) * is_) * k2 + (gk - k1)), gk


def _grad_sums(gk, y, mean, invstd):
    """float64 s1 = sum g * mask, s2 = sum g * mask * xhat per channel and the sums of their absolute terms"""
    g = gk.double()
    gx = g * ((y.double() - mean.double()) * invstd.double())
    return g.sum(0), gx.sum(0), g.abs().sum(0), gx.abs().sum(0)


def _tickets(ws):
    """the 64 first-level + 1 second-level ticket counters of pn2_bn_finish in a batch-norm workspace's head"""
    return ws.view(-1).view(torch.uint8)[:65 * 4].view(torch.int32).cpu().numpy()


def _folded(ws, c):
    d = ws.view(-1).view(torch.uint8)[:8 * (48 + 2 * c)].view(torch.float64)
    return d[48:48 + c].double(), d[48 + c:48 + 2 * c].double()


class Audit:
    """Wraps the tf_util entry points of the dense layers; every call is checked when it returns, against float64 of the
    operands it was given.  Only scalars are kept."""

    def __init__(self, pn2, flat, min_rows):
        self.pn2, self.tfu, self.lib = pn2, pn2.util.tf_util, pn2._lib.lib
        self.flat, self.min_rows = flat, min_rows  # flat: the trainer's flat gradient buffer
        self.cover = np.zeros(flat.numel(), bool)  # elements of the flat gradient a weight-gradient call added into
        self.rec = []        # (kind, shape, error, bound)
        self.bad = []        # what failed, as text
        self.gated = {"fwd": [], "dgrad_wide": [], "wide8": []}
        self.spans = []      # trace index ranges of the audited calls
        self.trace = []
        self.depth = 0
        self.counts = {}

    def ok(self, cond, what):
        if not cond:
            self.bad.append(what)

    def note(self, kind, shape, err, bound):
        self.rec.append((kind, shape, err, bound))
        self.ok(err <= bound, "%s %s: error %.3e > bound %.3e" % (kind, shape, err, bound))

    def _mark(self, t):
        base, p = self.flat.data_ptr(), t.data_ptr()
        if base <= p < base + 4 * self.flat.numel():
            assert t.is_contiguous()
            self.cover[(p - base) // 4:(p - base) // 4 + t.numel()] = True

    # ---- the yardsticks --------------------------------------------------------------------------------------------------
    def gemm(self, kind, x, w_t, got, onload, bias=None):
        """got = x @ w_t (+ bias): norm-relative error <= 1e-6 and <= 2x torch's fp32 product's (+2e-7 for operands formed on load)"""
        ref = x.double() @ w_t.double()
        yt = x @ w_t
        if bias is not None:
            ref, yt = ref + bias.double(), yt + bias
        e, et = _rel(got, ref), _rel(yt, ref)
        self.note(kind, (tuple(x.shape), w_t.shape[1]), e, min(1e-6, 2.0 * et + (2e-7 if onload else 1e-8)))

    def wgrad(self, kind, a, dy, delta, onload):
        """delta (what the call added to its output) = a^T dy.  Bound: recursive float32 summation of each element over the
        rows -- chunks of L rows per wave, then M chunk results added with atomics -- errs by at most (L + M) u sum|a_r dy_r|
        (first order), so ||err|| <= (L + M) u || |a|^T |dy| ||; and never more than 2x torch's fp32 product's error
        (+2e-7 for operands formed on load)."""
        rows, cin, cout = a.shape[0], a.shape[1], dy.shape[1]
        ref = a.double().t() @ dy.double()
        e, et = _rel(delta, ref), _rel(a.t() @ dy, ref)
        tm, tn = (2 if cin > 32 else 1), (4 if cout > 64 else (2 if cout > 32 else 1))
        waves = max(16, (2048 if wide8(rows, cin, cout, self.min_rows) else 1024) // ((cin + 32 * tm - 1) // (32 * tm) * ((cout + 32 * tn - 1) // (32 * tn))))
        chunk = max(32, (((rows + waves - 1) // waves) + 7) & ~7)
        depth = chunk + (rows + chunk - 1) // chunk
        absref = float((a.double().abs().t() @ dy.double().abs()).norm())
        bound = min(depth * U32 * absref / max(float(ref.norm()), 1e-300), 2.0 * et + (2e-7 if onload else 1e-8))
        self.note(kind, (rows, cin, cout), e, bound)

    def moments(self, y, consts, b, gamma, beta, decay, rm0, rv0, rm, rv):
        """what finish 2 published: save_mean, save_invstd, scale, shift and the running averages, against float64 moments of y"""
        yd = y.double()
        rows = y.shape[0]
        mean, var = yd.mean(0), yd.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + self.tfu.BN_EPSILON)
        sm, si, sc, sh = (t.double() for t in consts)
        ms = max(1.0, float(mean.abs().max()))
        sc_ref = gamma.double() * invstd
        sh_ref = beta.double() - mean * sc_ref
        errs = [float((sm - mean).abs().max()) / ms, float(((si - invstd) / invstd).abs().max()),
                float((sc - sc_ref).abs().max()) / float(sc_ref.abs().max()),
                float((sh - sh_ref).abs().max()) / max(1.0, float((beta.double().abs() + (mean * sc_ref).abs()).max()))]
        if rm is not None:
            m_out = mean + (0.0 if b is None else b.double())
            rm_ref = decay * rm0.double() + (1.0 - decay) * m_out
            rv_ref = decay * rv0.double() + (1.0 - decay) * var * (rows / (rows - 1.0))
            errs += [float((rm.double() - rm_ref).abs().max()) / max(1.0, float(rm_ref.abs().max())),
                     float((rv.double() - rv_ref).abs().max()) / max(1.0, float(rv_ref.abs().max()))]
        self.note("constants_fwd", (rows, y.shape[1]), max(errs), 1e-6)

    def folded_stats(self, ws, y):
        """the fold of the statistics (finish 1 and 2): sum y, sum y^2 per channel, relative to the sums of |terms|"""
        yd = y.double()
        s1, s2 = _folded(ws, y.shape[1])
        e = max(float(((s1 - yd.sum(0)).abs() / yd.abs().sum(0).clamp_min(1e-300)).max()),
                float(((s2 - (yd * yd).sum(0)).abs() / (yd * yd).sum(0).clamp_min(1e-300)).max()))
        self.note("fold_fwd", tuple(y.shape), e, 1e-6)

    def grad_constants(self, kind, rows, c, coef, dgamma, dbeta, sums, gamma, beta, mean, invstd):
        """coef (6, c) = sc, sh, mean, invstd (bit for bit), k1 = s1 / rows, k2 = s2 / rows; dbeta = s1, dgamma = s2"""
        s1, s2, a1, a2 = sums
        sc, sh = _bn_affine(gamma, beta, mean, invstd)
        self.ok(torch.equal(coef[0], sc) and torch.equal(coef[1], sh) and torch.equal(coef[2], mean) and torch.equal(coef[3], invstd),
                "%s (%d, %d): coef[0:4] are not sc, sh, mean, invstd" % (kind, rows, c))
        a1, a2 = a1.clamp_min(1e-30), a2.clamp_min(1e-30)
        e = max(float(((coef[4].double() * rows - s1).abs() / a1).max()), float(((coef[5].double() * rows - s2).abs() / a2).max()),
                float(((dbeta.double() - s1).abs() / a1).max()), float(((dgamma.double() - s2).abs() / a2).max()))
        self.note(kind, (rows, c), e, 1e-6)

    def grad_fold(self, ws, rows, c, sums):
        s1, s2, a1, a2 = sums
        f1, f2 = _folded(ws, c)
        e = max(float(((f1 - s1).abs() / a1.clamp_min(1e-30)).max()), float(((f2 - s2).abs() / a2.clamp_min(1e-30)).max()))
        self.note("fold_dgrad", (rows, c), e, 1e-6)

    def tickets(self, ws, what, expect):
        t = _tickets(ws)
        n = int(t[:64].sum())
        self.ok(n > 0 and int(t[64]) == min(64, n), "%s: tickets %d / %d" % (what, n, int(t[64])))
        if expect is not None:
            self.ok(n == expect, "%s: %d tickets drawn, the streaming launch has %d workgroups" % (what, n, expect))

    # ---- the link below: the finish a data-gradient launch ran for the layer under it ------------------------------------
    def below(self, what, dx, link, kind, pws, expect_wg):
        rows, c = dx.shape
        sc, sh = _bn_affine(link.gamma, link.beta, link.mean, link.invstd)
        lin = link.y.double() * sc.double() + sh.double()
        gk = torch.where(lin > 0, dx, torch.zeros_like(dx)) if link.relu else dx
        sums = _grad_sums(gk, link.y, link.mean, link.invstd)
        del lin, gk
        if kind == 3:
            self.grad_constants("constants_dgrad", rows, c, link.coef, link.dgamma, link.dbeta, sums, link.gamma, link.beta,
                                link.mean, link.invstd)
        self.grad_fold(pws, rows, c, sums)
        self.tickets(pws, what, expect_wg)

    # ---- wrappers -------------------------------------------------------------------------------------------------------
    def install(self):
        tfu, A = self.tfu, self
        self.orig = {k: getattr(tfu, k) for k in ("hip_matmul_bn_stats_fin", "hip_matmul_bn_stats", "hip_matmul_bn_stats_xf", "hip_matmul",
                                                   "hip_linear_narrow", "_hip_dgrad_fin", "hip_linear_dgrad", "hip_linear_dgrad_linked",
                                                   "_hip_bwd_fused", "_hip_wgrad", "_hip_wgrad_gx", "_hip_wgrad_into", "_bn_grad_constants")}
        O = self.orig

        def wrap(name, audit):
            def f(*args, **kw):
                if A.depth:  # called from inside another audited entry point: that one checks it
                    return O[name](*args, **kw)
                pre = audit.get("pre", lambda *a, **k: None)(*args, **kw)
                tr = A.lib.trace
                n0 = len(tr)
                A.depth += 1
                try:
                    out = O[name](*args, **kw)
                finally:
                    A.depth -= 1
                launches = [(t[0], t[1]) for t in tr[n0:]]
                A.spans.append((n0, len(tr)))
                A.lib.trace = None  # the witness launches below are not part of the step
                try:
                    audit["post"](out, launches, pre, *args, **kw)
                finally:
                    A.lib.trace = tr
                return out
            setattr(tfu, name, f)

        for name, fn in (("hip_matmul_bn_stats_fin", self._fwd_fin), ("hip_matmul_bn_stats", self._fwd_stats),
                         ("hip_matmul_bn_stats_xf", self._fwd_stats_xf), ("hip_matmul", self._fwd_plain),
                         ("hip_linear_narrow", self._fwd_narrow), ("_hip_dgrad_fin", self._dgrad_fin),
                         ("hip_linear_dgrad", self._dgrad_plain), ("hip_linear_dgrad_linked", self._dgrad_linked),
                         ("_hip_bwd_fused", self._bwd_fused), ("_hip_wgrad", self._wgrad), ("_hip_wgrad_gx", self._wgrad_gx),
                         ("_hip_wgrad_into", self._wgrad_into), ("_bn_grad_constants", self._bn_constants)):
            wrap(name, fn())

    def uninstall(self):
        for k, v in self.orig.items():
            setattr(self.tfu, k, v)

    def count(self, kind):
        self.counts[kind] = self.counts.get(kind, 0) + 1

    def _fwd_gate(self, launches, x, w):
        for nm, ints in launches:
            if nm in FWD_LAUNCHES:
                rows, cin, cout = ints[:3]
                if fwd_narrow_fits(rows, cin, cout, self.min_rows) and _aligned(x, w):
                    self.gated["fwd"].append((rows, cin, cout))
                    return True
        return False

    def _fwd_witness(self, x_raw, w, xf, y, entry):
        """the same entry point on the operands padded by one row (a shape the streaming kernel refuses), fresh workspace,
        finish 1: y bit for bit on the shared rows"""
        xp = torch.cat([x_raw, x_raw[:1]])
        ws = torch.zeros(self.lib.pn2_bn_workspace_bytes(w.shape[1]) // 8, dtype=torch.float64, device=y.device)
        yp = entry(xp, w, ws, xf)
        self.ok(torch.equal(yp[:y.shape[0]], y), "forward %s: streaming y != tiled y" % (tuple(y.shape),))

    def _fwd_fin(self):
        def pre(x2d, w, ws, xf, finish, gamma=None, beta=None, b=None, decay=0.0, running_mean=None, running_var=None):
            return (running_mean.clone(), running_var.clone()) if running_mean is not None else (None, None)

        def post(out, launches, pre_, x2d, w, ws, xf, finish, gamma=None, beta=None, b=None, decay=0.0, running_mean=None, running_var=None):
            y, consts = out
            self.count("fwd")
            x = x2d if xf is None else _fma(x2d, xf[0], xf[1], xf[2])
            self.gemm("fwd", x, w, y, xf is not None)
            del x
            if finish == 2:
                self.moments(y, consts, b, gamma, beta, decay, pre_[0], pre_[1], running_mean, running_var)
            self.folded_stats(ws, y)
            gated = self._fwd_gate(launches, x2d, w)
            self.tickets(ws, "forward %s" % (tuple(y.shape),), fwd_stream_workgroups(y.shape[0], x2d.shape[1]) if gated else None)
            if gated:
                self._fwd_witness(x2d, w, xf, y, lambda xp, w_, ws_, xf_: self.orig["hip_matmul_bn_stats_fin"](xp, w_, ws_, xf_, 1)[0])
        return dict(pre=pre, post=post)

    def _fwd_stats(self):
        def post(y, launches, pre_, x2d, w, ws):
            self.count("fwd")
            self.gemm("fwd", x2d, w, y, False)
            if self._fwd_gate(launches, x2d, w):
                self._fwd_witness(x2d, w, None, y, lambda xp, w_, ws_, xf_: self.orig["hip_matmul_bn_stats"](xp, w_, ws_))
        return dict(post=post)

    def _fwd_stats_xf(self):
        def post(y, launches, pre_, x_raw, w, ws, sc, sh, relu):
            self.count("fwd")
            self.gemm("fwd", _fma(x_raw, sc, sh, relu), w, y, True)
            if self._fwd_gate(launches, x_raw, w):
                self._fwd_witness(x_raw, w, (sc, sh, relu), y,
                                  lambda xp, w_, ws_, xf_: self.orig["hip_matmul_bn_stats_xf"](xp, w_, ws_, *xf_))
        return dict(post=post)

    def _fwd_plain(self):
        def post(y, launches, pre_, x2d, w):
            self.count("fwd")
            self.gemm("fwd", x2d, w, y, False)
        return dict(post=post)

    def _fwd_narrow(self):
        def post(y, launches, pre_, x2d, w, b=None):
            if y is not None:
                self.count("fwd")
                self.gemm("fwd", x2d, w, y, False, bias=b)
        return dict(post=post)

    def _dgrad_checks(self, what, dy, w, dx, onload, link, launches, gx):
        """dx against float64 of (dy @ w^T); the finish the launch ran for the layer below; the dgrad_wide gate"""
        self.gemm(what, dy, w.t(), dx, onload)
        kind = 0
        for nm, ints in launches:
            if nm in ("pn2_linear_dgrad_fin", "pn2_linear_bwd_fused", "pn2_linear_dgrad_gx", "pn2_linear_dgrad_bn_grad_stats"):
                if nm in ("pn2_linear_dgrad_fin", "pn2_linear_bwd_fused"):
                    kind = ints[-1]
                rows, cin, cout = ints[:3]
                if gx is not None and nm in ("pn2_linear_dgrad_fin", "pn2_linear_dgrad_gx"):
                    y, dz, coef, relu, pool, zmax, ties = gx
                    if dgrad_wide_fits(rows, cin, cout, pool, self.min_rows) and _aligned(y, dz, coef, w, zmax, ties):
                        self.gated["dgrad_wide"].append((rows, cin, cout, pool))
                        return kind, True
        return kind, False

    def _dgrad_witness(self, gx, w, dx, link):
        """the same entry point on the first 65504 rows (below the streaming threshold, a multiple of 32), the layer below's
        sums into a fresh workspace (finish 1): dx bit for bit"""
        L, P = self.lib, self.pn2._lib.ptr
        y, dz, coef, relu, pool, zmax, ties = gx
        n = 65504
        ties = ties[0] if (ties is not None and ties.dim() == zmax.dim() + 1) else ties
        ng = n // pool if pool else n
        d = torch.empty(n, w.shape[0], device=dx.device)
        bel = (None, None, None, None, None, 0, None, 0, 0, None, None, None)
        if link is not None:
            nb = L.pn2_bn_workspace_bytes(w.shape[0])
            ws = torch.zeros(nb // 8, dtype=torch.float64, device=dx.device)
            bel = (P(link.y[:n]), P(link.gamma), P(link.beta), P(link.mean), P(link.invstd), int(link.relu), P(ws), nb, 1, None, None, None)
        rc = L.pn2_linear_dgrad_fin(n, w.shape[0], w.shape[1], None, P(y[:n]), P(dz[:ng]), P(coef), int(relu), int(pool),
                                    P(None if zmax is None else zmax[:ng].contiguous()), P(None if ties is None else ties[:ng].contiguous()),
                                    P(w.contiguous()), P(d), *bel, self.pn2._lib.stream_ptr())
        self.ok(rc == 0 and torch.equal(d, dx[:n]), "dgrad %s: streaming dx != tiled dx (rc %d)" % (tuple(dx.shape), rc))

    def _dgrad_fin(self):
        def pre(dy, gx, w, link):
            return None

        def post(dx, launches, pre_, dy, gx, w, link):
            self.count("dgrad")
            dym = dy if gx is None else dy_on_load(*gx)[0]
            kind, gated = self._dgrad_checks("dgrad" if gx is None else "dgrad_gx", dym, w, dx, gx is not None, link, launches, gx)
            del dym
            if link is not None:
                self.below("dgrad %s" % (tuple(dx.shape),), dx, link, kind, link.ws, dgrad_wide_workgroups(dx.shape[0]) if gated else None)
            if gated:
                self._dgrad_witness(gx, w, dx, link)
        return dict(pre=pre, post=post)

    def _dgrad_plain(self):
        def post(dx, launches, pre_, dy, w):
            self.count("dgrad")
            self.gemm("dgrad", dy, w.t(), dx, False)
        return dict(post=post)

    def _dgrad_linked(self):
        def post(dx, launches, pre_, dy, w, link):
            self.count("dgrad")
            kind, _ = self._dgrad_checks("dgrad", dy, w, dx, False, link, launches, None)
            self.below("dgrad %s" % (tuple(dx.shape),), dx, link, kind, link.ws, None)
        return dict(post=post)

    def _wgrad_target(self, w):
        """the tensor a weight-gradient call of parameter w adds into, cloned: its flat-gradient slice, else zero (the zero arena /
        a fresh zero fill)"""
        gv = self.tfu.get_default_store().grad_view(w)
        return None if gv is None else gv.clone()

    def _delta(self, out, before):
        d = out if before is None else out - before
        self._mark(out)
        return d

    def _bwd_fused(self):
        def pre(x2d, xf, y, dz, coef, relu, pool, zmax, ties, w, link):
            return self._wgrad_target(w)

        def post(out, launches, before, x2d, xf, y, dz, coef, relu, pool, zmax, ties, w, link):
            if out is None:
                return
            dx, dw = out
            self.count("dgrad")
            self.count("wgrad")
            dy = dy_on_load(y, dz, coef, relu, pool, zmax, ties)[0]
            kind, _ = self._dgrad_checks("dgrad_gx", dy, w, dx, True, link, launches, None)
            a = x2d if xf is None else _fma(x2d, xf[0], xf[1], xf[2])
            self.wgrad("wgrad_gx", a, dy, self._delta(dw, before), True)
            del a, dy
            if link is not None:
                self.below("bwd_fused %s" % (tuple(dx.shape),), dx, link, kind, link.ws, None)
        return dict(pre=pre, post=post)

    def _wgrad_gate(self, launches):
        for nm, ints in launches:
            if nm in WGRAD_LAUNCHES and wide8(ints[0], ints[1], ints[2], self.min_rows):
                self.gated["wide8"].append(tuple(ints[:3]))

    def _wgrad(self):
        def pre(x2d, dy, w, xf=None):
            return self._wgrad_target(w)

        def post(dw, launches, before, x2d, dy, w, xf=None):
            self.count("wgrad")
            a = x2d if xf is None else _fma(x2d, xf[0], xf[1], xf[2])
            self.wgrad("wgrad", a, dy, self._delta(dw, before), xf is not None)
            self._wgrad_gate(launches)
        return dict(pre=pre, post=post)

    def _wgrad_gx(self):
        def pre(x2d, xf, y, dz, coef, relu, pool, zmax, ties, w):
            return self._wgrad_target(w)

        def post(dw, launches, before, x2d, xf, y, dz, coef, relu, pool, zmax, ties, w):
            self.count("wgrad")
            a = x2d if xf is None else _fma(x2d, xf[0], xf[1], xf[2])
            dy = dy_on_load(y, dz, coef, relu, pool, zmax, ties)[0]
            self.wgrad("wgrad_gx", a, dy, self._delta(dw, before), True)
            self._wgrad_gate(launches)
        return dict(pre=pre, post=post)

    def _wgrad_into(self):
        def pre(x2d, dy, dw_rows):
            return dw_rows.clone()

        def post(_, launches, before, x2d, dy, dw_rows):
            self.count("wgrad_into")
            self.wgrad("wgrad_into", x2d, dy, self._delta(dw_rows, before), False)
            self._wgrad_gate(launches)
        return dict(pre=pre, post=post)

    def _bn_constants(self):
        def post(out, launches, pre_, dz, y, gamma, beta, save_mean, save_invstd, relu, pool, zmax, ties, lk):
            if not any(nm == "pn2_bn_grad_constants" for nm, _ in launches):
                return  # published by the consumer's data-gradient launch (finish 3): checked there
            self.count("bn_grad_constants")
            coef, dgamma, dbeta = out
            sc, sh = _bn_affine(gamma, beta, save_mean, save_invstd)
            c6 = (sc, sh, save_mean, save_invstd, coef[4], coef[5])
            gk = dy_on_load(y, dz, c6, relu, pool, zmax, ties)[1]
            self.grad_constants("constants_bn", y.shape[0], y.shape[1], coef, dgamma, dbeta, _grad_sums(gk, y, save_mean, save_invstd),
                                gamma, beta, save_mean, save_invstd)
        return dict(post=post)


SIZES = {"full": (16, 8192, None), "small": (8, 2048, dict(l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16))}
# pinned from the trace: (rows, cin, cout) of the calls that pass each gate at the full size
FULL_GATED = {
    # SA1's 32-channel layers (16 x 1024 x 32 rows), SA2's second and third layer, FP4's two 128 -> 128 layers, the head's fc1
    "fwd": sorted([(524288, 32, 32), (524288, 32, 64), (131072, 64, 64), (131072, 64, 128), (131072, 128, 128), (131072, 128, 128),
                   (131072, 128, 128)]),
    # FP4's two 128 -> 128 layers, fc1, SA2's pooled last layer
    "dgrad_wide": sorted([(131072, 128, 128, 0), (131072, 128, 128, 0), (131072, 128, 128, 0), (131072, 64, 128, 32)]),
    "wide8": sorted([(131072, 128, 128), (131072, 128, 128), (131072, 128, 128), (131072, 64, 128)]),
}
SMALL_GATED = {"fwd": sorted([(65536, 32, 32), (65536, 32, 64)]), "dgrad_wide": [], "wide8": []}


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("size", ["full", "small"])
def test_every_kernel_call_of_a_training_step_against_float64(pn2, cuda, size, step):
    """An eager Trainer step (capture=False) with every dense-layer entry point of util/tf_util.py checked as it returns, against
    float64 of its own operands (operands formed on load are materialised with the kernels' float32 fma forms):
      * forward / data-gradient products: norm-relative error <= 1e-6 and <= 2x torch's fp32 product (+2e-7 on load);
      * weight gradients -- the DELTA a call added to its output (on every step that is the parameter's slice of the flat
        gradient buffer, zero-filled once per step): <= (L + M) u || |a|^T |dy| || / ||a^T dy||, the first-order bound of float32
        summation over the rows in chunks of L rows and M chunk results (Audit.wgrad), and <= 2x torch's error (+2e-7 on load);
      * published batch-norm constants (finish 2: mean, invstd, scale, shift, running averages; finish 3 and pn2_bn_grad_constants:
        coef (6, c), dgamma, dbeta) and the folded sums of finish 1: <= 1e-6 relative (sums: to the sum of |terms| per channel);
        coef[0:4] bit for bit;
      * the ticket counters each finish left in its workspace head: one per workgroup, the streaming launches' exact count.
    Step 1 runs before the trainer's zero arena exists (every workspace zero-fills itself); step 3 -- a fresh trainer's third,
    after two unaudited steps -- takes every accumulator and ticket head from the arena.  Both write the weight gradients into the
    flat buffer (grad_view).  The calls that pass the streaming gates (csrc/pn2_common.h PN2_STREAM_MIN_ROWS) are pinned, and each
    gated forward / dgrad_wide call is re-run where the tiled kernel takes it: bit-identical.
    Measured on the MI355X at the full size, worst over steps 1 and 3 (the bound of that call in brackets): forward 2.6e-7 (5.3e-7),
    data gradient 2.9e-7 (5.9e-7), formed on load 4.1e-7 (1e-6); weight gradient 1.7e-7 (5.3e-7), formed on load 3.1e-7 (2.5e-6),
    hoisted row blocks 3.5e-7 (1.5e-6); constants: forward 1.1e-7, finish 3 1.3e-8, pn2_bn_grad_constants 3.4e-8; folded sums
    1.6e-15 (forward) and 1.1e-8 (data gradient) -- all against 1e-6.  The small size measures figures of the same order."""
    tfu = pn2.util.tf_util
    b, n, small = SIZES[size]
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    if small:
        hp.update(small)
    batches = [_batch(cuda, b, n, seed=s) for s in range(step)]
    tr = pn2.train.Trainer(hp, 9, store=tfu.VariableStore(device=cuda, seed=5), capture=False)
    tr._lazy_init(batches[0][0])  # what the first train_step does first (variables, flat buffers): before the wrappers go in
    for i in range(step - 1):
        assert np.isfinite(tr.train_step(*batches[i]))
    assert (tr.store.zero_arena is not None and tr.store.zero_arena.buf is not None) == (step > 1)
    min_rows = stream_min_rows()
    A = Audit(pn2, tr.bucket.flat, min_rows)
    A.install()
    A.lib.trace = A.trace
    try:
        loss = tr.train_step(*batches[step - 1])
    finally:
        A.lib.trace = None
        A.uninstall()
    torch.cuda.synchronize()
    assert np.isfinite(loss)

    kinds = sorted({r[0] for r in A.rec})
    print("\n[%s, step %d] %d calls audited" % (size, step, len(A.rec)))
    for k in kinds:
        rs = [r for r in A.rec if r[0] == k]
        w = max(rs, key=lambda r: r[2] / max(r[3], 1e-300))
        print("  %-16s %3d calls, worst error %.2e (bound %.2e) at %s" % (k, len(rs), w[2], w[3], w[1]))
    print("  entry points: %s" % sorted(A.counts.items()))
    print("  gated: fwd %s; dgrad_wide %s; wide8 %s" % (sorted(A.gated["fwd"]), sorted(A.gated["dgrad_wide"]), sorted(A.gated["wide8"])))
    assert not A.bad, "\n".join(A.bad[:20])

    # coverage: every dense-layer launch of the step lies inside an audited call; each layer in forward, data and weight gradient
    inside = np.zeros(len(A.trace), bool)
    for s, e in A.spans:
        inside[s:e] = True
    stray = [t[0] for t, i in zip(A.trace, inside) if t[0] in GEMM_LAUNCHES and not i]
    assert not stray, stray
    hoisted = 4  # the first layers of SA2, SA3, SA4 and FP4 (tf_util._TrainHoistedBnRelu)
    assert A.counts.get("fwd") == 22 and A.counts.get("dgrad") == 22, A.counts  # 23 layers; SA1's first is one launch with its front end
    assert A.counts.get("wgrad_into") == 2 * hoisted and A.counts.get("wgrad") == 23 - hoisted + 1, A.counts  # + fc2's bias
    store = tr.store
    for name, p in store.params.items():
        if name.endswith("weights") or name == "fc2/biases":
            _, off, k = store.grad_map[p.data_ptr()]
            assert A.cover[off:off + k].all(), name
    # the streaming kernels: which calls pass the gates
    want = FULL_GATED if size == "full" else SMALL_GATED
    for fam in ("fwd", "dgrad_wide", "wide8"):
        assert sorted(A.gated[fam]) == want[fam], (fam, sorted(A.gated[fam]))
