"""The training step's elementwise tail (csrc/pn2_train.hip, csrc/pn2_pool.hip) at its edges, entry point by entry point:
dropout bit for bit against the host model of its draw, ReLU gradient and multi-copy byte for byte, weighted cross-entropy,
Adam and group pooling against float64 -- at sizes around the vector width and past the 4096-block grid cap, on views that
start off a 16-byte boundary, and with the special values (signed zero, denormals, inf, NaN) a happy-path test never draws.

"Unaligned" is an ordinary view into a larger tensor; the elements of that tensor on both sides of the view must stay as
they were.  Where a float32 result is compared with float64, the bound is MEASURED: the same formula is evaluated in float32
numpy in the kernel's order, its worst error against float64 over the same cases is taken, and the kernel may be 4 times
that far off (device expf / logf are within 1-2 ulp of the host's, and a block reduction sums in another order)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_ref as D  # noqa: E402
from test_train_gpu import adam_ref_step  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 4096 * 256            # grid_1d / pool_grid: at most 4096 blocks of 256 threads, then grid-stride
HEAD = 16 * 8192 * 128      # the full-size head activation that dropout sees
PAD_F, PAD_B = 7.25, 0xA5   # what the margins around a view hold
MARGIN = 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class View:
    """`n` elements inside a larger 1-D tensor, `off` elements past a 16-byte boundary, with padded margins on both sides"""

    def __init__(self, dev, n, dtype, off=0, data=None):
        import torch
        item = torch.empty((), dtype=dtype).element_size()
        self.lead, self.n = 16 // item + off, n
        self.pad = PAD_B if dtype == torch.uint8 else PAD_F
        self.base = torch.full((self.lead + n + 16 // item + MARGIN,), self.pad, dtype=dtype, device=dev)
        self.t = self.base[self.lead:self.lead + n]
        assert self.t.data_ptr() % 16 == (off * item) % 16
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.t.data_ptr())

    def get(self):
        """the view's content, after checking that the kernel left both margins alone"""
        b = self.base.cpu().numpy()
        assert (b[:self.lead] == self.pad).all() and (b[self.lead + self.n:] == self.pad).all(), "wrote outside its view"
        return b[self.lead:self.lead + self.n].copy()


def specials(x):
    """plant -0.0, the smallest denormal, inf and NaN among the first elements (as many as fit)"""
    s = np.array([-0.0, 1e-45, np.inf, np.nan, -np.inf, 0.0], np.float32)
    k = min(len(s), x.size)
    x[:k] = s[:k]
    if x.size > 2 * len(s):
        x[-len(s):] = s[::-1]  # ... and among the last ones: the tail of the last vector / the last block
    return x


# ------------------------------------------------------------------------------------------------------------------ dropout
def run_dropout(L, dev, x, keep, seed, step, offs=(0, 0, 0), dy=None):
    """pn2_dropout, then pn2_dropout_grad with the mask it wrote (same alignment) -> y, mask, dx as numpy"""
    import torch
    n = x.size
    vx, vy, vm = View(dev, n, torch.float32, offs[0], x), View(dev, n, torch.float32, offs[1]), View(dev, n, torch.uint8, offs[2])
    state = torch.tensor([seed, step], dtype=torch.int64, device=dev)
    L.launch("pn2_dropout", state, n, vx.ptr(), float(keep), L.ptr(state), vy.ptr(), vm.ptr())
    y, mask = vy.get(), vm.get()
    assert np.array_equal(bits(vx.get()), bits(x))
    dx = None
    if dy is not None:
        vdy, vdx = View(dev, n, torch.float32, offs[0], dy), View(dev, n, torch.float32, offs[1])
        L.launch("pn2_dropout_grad", state, n, vdy.ptr(), vm.ptr(), float(keep), vdx.ptr())
        dx = vdx.get()
        assert np.array_equal(vm.get(), mask)
    return y, mask, dx


def check_dropout(L, dev, n, keep, seed, step, offs=(0, 0, 0), rs_seed=0):
    rs = np.random.RandomState(rs_seed)
    x, dy = specials(rs.randn(n).astype(np.float32)), specials(rs.randn(n).astype(np.float32))[::-1].copy()
    y, mask, dx = run_dropout(L, dev, x, keep, seed, step, offs, dy)
    kept = D.keep_bits(seed, step, n, keep)
    what = "n=%d keep=%g seed=%d step=%d offs=%s" % (n, keep, seed, step, offs)
    bad = np.flatnonzero(mask != kept.astype(np.uint8))
    assert bad.size == 0, "%s: mask differs from the host model at %s ..." % (what, bad[:8])
    for got, src, name in ((y, x, "y"), (dx, dy, "dx")):
        bad = np.flatnonzero(bits(got) != bits(D.apply(src, kept, keep)))
        assert bad.size == 0, "%s: %s differs at %s ..." % (what, name, bad[:8])
    return y, mask


SEEDS = [(9, 0), (0x7FEDCBA900000000, 1), (0x123456789ABCDEF, 2 ** 40), (-3, 1), (-0x0FEDCBA987654321, 2 ** 40), (D.KEEP_ONE_SEED, 0)]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 1027])
@pytest.mark.parametrize("keep", [0.5, 0.9, 0.1, 1.0])
def test_dropout_bit_for_bit_small(pn2, cuda, n, keep):
    """Mask, y and dx of pn2_dropout / pn2_dropout_grad equal the host model (tests/dropout_ref.py) bit for bit: random normal
    input with -0.0, a denormal, +-inf and NaN (a dropped NaN gives 0), seeds with the high word set and negative seeds, steps
    0, 1 and 2**40, and each of x / y / mask in turn one element off a 16-byte boundary (the scalar variant, chosen for each
    reason separately)."""
    for seed, step in SEEDS:
        check_dropout(pn2._lib, cuda, n, keep, seed, step, rs_seed=n)
    for offs in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 2, 1)]:
        check_dropout(pn2._lib, cuda, n, keep, 0x7FEDCBA900000009, 2 ** 40, offs, rs_seed=n)


@pytest.mark.parametrize("n,offs", [(CAP * 4 + 4, (0, 0, 0)), (CAP + 1, (0, 0, 0)), (CAP * 4 + 4, (1, 0, 0)), (HEAD, (0, 0, 0))])
def test_dropout_bit_for_bit_past_the_grid_cap(pn2, cuda, n, offs):
    """the first sizes whose grid-stride loop runs twice (vector: n / 4 > 4096 * 256; scalar: n > 4096 * 256, by an odd n and by
    an unaligned x) and the full-size head activation"""
    check_dropout(pn2._lib, cuda, n, 0.5, -0x0FEDCBA987654321, 2 ** 40, offs)
    if n == HEAD:
        check_dropout(pn2._lib, cuda, n, 0.9, 9, 1, offs)


def test_dropout_vector_and_scalar_variants_draw_the_same(pn2, cuda):
    """the draw of element i does not depend on the variant: same bytes on the common prefix for the same (seed, step)"""
    rs = np.random.RandomState(5)
    x = rs.randn(1028).astype(np.float32)
    for keep in (0.5, 0.9, 0.1):
        for seed, step in SEEDS[:3]:
            yv, mv, _ = run_dropout(pn2._lib, cuda, x, keep, seed, step)                       # n % 4 == 0, aligned: vector
            ys, ms, _ = run_dropout(pn2._lib, cuda, x[:1027], keep, seed, step)                # n % 4 != 0: scalar
            yu, mu, _ = run_dropout(pn2._lib, cuda, x, keep, seed, step, offs=(0, 0, 1))       # unaligned mask: scalar
            assert np.array_equal(bits(yv)[:1027], bits(ys)) and np.array_equal(mv[:1027], ms)
            assert np.array_equal(bits(yv), bits(yu)) and np.array_equal(mv, mu)
            assert 0 < mv.sum() < 1028


def test_dropout_keep_prob_one_keeps_the_all_ones_draw(pn2, cuda):
    """keep_prob = 1 with the seed for which element 0 of step 0 draws 0xFFFFFFFF (constructed and verified in
    test_train_tail_cpu.py): element 0 is kept and y == x everywhere, in both variants.  A `draw < 0xFFFFFFFF` rule drops it."""
    rs = np.random.RandomState(6)
    for n, offs in [(1028, (0, 0, 0)), (1027, (0, 0, 0)), (1, (0, 0, 0)), (1028, (1, 0, 0))]:
        x = rs.randn(n).astype(np.float32) + 3.0
        dy = rs.randn(n).astype(np.float32)
        y, mask, dx = run_dropout(pn2._lib, cuda, x, 1.0, D.KEEP_ONE_SEED, 0, offs, dy)
        assert mask[0] == 1 and y[0] == x[0], (n, offs)
        assert (mask == 1).all() and np.array_equal(bits(y), bits(x)) and np.array_equal(bits(dx), bits(dy))


# ---------------------------------------------------------------------------------------------------------------- relu grad
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 1027, 1028, CAP * 4 + 4, CAP + 1])
def test_relu_grad_vs_numpy(pn2, cuda, n):
    """dx = dz where z > 0, else +0: z holds -0.0, +0.0, the smallest denormal (positive: passes), NaN (not greater than 0:
    blocks) and +-inf; both variants, each pointer in turn off a 16-byte boundary, dx aliasing dz, sizes past the grid cap.
    A select, so the comparison is bit for bit."""
    import torch
    L = pn2._lib
    rs = np.random.RandomState(n % 1000)
    z = rs.randn(n).astype(np.float32)
    sp = np.array([-0.0, 0.0, 1e-45, np.nan, np.inf, -np.inf, -1e-45], np.float32)
    z[:min(n, len(sp))] = sp[:min(n, len(sp))]
    if n > 16:
        z[-7:] = sp[::-1]
    dz = rs.randn(n).astype(np.float32)
    dz[dz == 0] = 1.0
    if n > 16:
        dz[8:12] = [np.nan, -0.0, np.inf, 1e-45]
        z[8:12] = [1.0, 2.0, -1.0, 3.0]
    with np.errstate(invalid="ignore"):
        ref = np.where(z > 0, dz, np.float32(0))
    for offs in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 3, 1)] if n < CAP else [(0, 0, 0), (0, 1, 0)]:
        vz, vdz, vdx = View(cuda, n, torch.float32, offs[0], z), View(cuda, n, torch.float32, offs[1], dz), View(cuda, n, torch.float32, offs[2])
        L.launch("pn2_relu_grad", vz.t, n, vz.ptr(), vdz.ptr(), vdx.ptr())
        assert np.array_equal(bits(vdx.get()), bits(ref)), (n, offs)
        assert np.array_equal(bits(vdz.get()), bits(dz)) and np.array_equal(bits(vz.get()), bits(z))
        L.launch("pn2_relu_grad", vz.t, n, vz.ptr(), vdz.ptr(), vdz.ptr())  # in place: dx aliases dz
        assert np.array_equal(bits(vdz.get()), bits(ref)), (n, offs, "aliased")


# ------------------------------------------------------------------------------------------------------------ cross-entropy
CE_SHAPES = [(r, c) for c in (1, 2, 9, 13, 64) for r in (1, 255, 256, 257, 131072)] + [(CAP // 64 + 1, 64)]
CE_SCALES = (1.0, 30.0, 1e4)
GOUT = 2.5


def ce_case(rows, c, scale, seed, minus_inf_label=False):
    """logits, int64 labels, weights.  From 8 rows and 2 classes on: a row of equal logits, a row with one -inf (probability
    exactly 0, finite gradient), weights 0, a denormal, a negative one and 1e6.  minus_inf_label: one more row whose label
    sits on its -inf entry (loss +inf)."""
    rs = np.random.RandomState(seed)
    logits = (rs.randn(rows, c) * scale).astype(np.float32)
    labels = rs.randint(0, c, rows).astype(np.int64)
    w = (rs.random_sample(rows) * 2).astype(np.float32)
    w[: rows // 7] = 0.0
    if rows >= 8:
        logits[-1] = logits[-1, 0]
        w[-8:] = [0.5, 0.0, 1e-40, -0.75, 1e6, 1.25, 1.0, 1.5]
        if c >= 2:
            logits[-2, c - 1] = -np.inf
            labels[-2] = 0
            if minus_inf_label:
                logits[-3, c - 1] = -np.inf
                labels[-3] = c - 1
    return logits, labels, w


def ce_float64(oracle, logits, labels, w):
    """The documented loss in float64: a row with a label outside [0, C) counts as weight 0.  -> loss
    (oracle.weighted_sparse_ce), lse, d loss / d logits for upstream gradient 1 (float64 torch autograd), and the scales the
    float32 errors are measured in (loss: sum |w| max(1, |lse|, |z_label|) / nz; gradient: |w_r| / nz per row)."""
    import torch
    rows, c = logits.shape
    valid = (labels >= 0) & (labels < c)
    lab = np.where(valid, labels, 0)
    we = np.where(valid, w, np.float32(0)).astype(np.float64)
    with np.errstate(all="ignore"):
        loss = oracle.weighted_sparse_ce(logits.astype(np.float64).reshape(1, rows, c), lab.reshape(1, rows), we.reshape(1, rows))
    nz = max(1, int(np.count_nonzero(we)))
    z = torch.from_numpy(logits).double().requires_grad_(True)
    lse = torch.logsumexp(z, 1)
    ce = lse - z.gather(1, torch.from_numpy(lab).reshape(-1, 1)).reshape(-1)
    (ce * torch.from_numpy(we)).sum().div(nz).backward()
    lse = lse.detach().numpy()
    zl = logits[np.arange(rows), lab].astype(np.float64)
    zl = np.where(np.isfinite(zl), zl, 0.0)
    loss_scale = float((np.abs(we) * np.maximum(1.0, np.maximum(np.abs(lse), np.abs(zl)))).sum() / nz)
    return loss, lse, z.grad.numpy(), max(loss_scale, 1e-30), np.maximum(np.abs(we) / nz, 1e-30).reshape(-1, 1), valid


def ce_float32(logits, labels, w, gout):
    """the kernels' formula in float32 numpy: max, exp, sum in class order, log; w * ce per row summed in float64"""
    f = np.float32
    rows, c = logits.shape
    valid = (labels >= 0) & (labels < c)
    lab = np.where(valid, labels, 0)
    with np.errstate(all="ignore"):
        mx = logits.max(axis=1)
        se = np.zeros(rows, f)
        for k in range(c):
            se = se + np.exp(logits[:, k] - mx)
        lse = (mx + np.log(se)).astype(f)
        per = np.where(valid, w * (lse - logits[np.arange(rows), lab]), f(0)).astype(f)
        nz = max(1, int(np.count_nonzero(np.where(valid, w, f(0)))))
        loss = f(per.astype(np.float64).sum() / nz)
        scale = f(gout) / f(nz)
        onehot = (np.arange(c)[None, :] == lab[:, None]).astype(f)
        grad = np.where(valid[:, None], (scale * w)[:, None] * (np.exp(logits - lse[:, None]) - onehot), f(0)).astype(f)
    return loss, lse, grad


def ce_kernel(L, dev, logits, labels, w, ldt, gout):
    """direct ABI calls with state tensors of the test's own -> loss, lse, dlogits, acc"""
    import torch
    rows, c = logits.shape
    tl, tw = torch.from_numpy(logits).to(dev), torch.from_numpy(w).to(dev)
    with np.errstate(all="ignore"):
        tlab = torch.from_numpy(labels.astype(ldt)).to(dev)
    lse = torch.full((rows,), PAD_F, device=dev)
    acc = torch.full((2,), 123.0, dtype=torch.float64, device=dev)  # zeroed by the callee
    loss = torch.full((), PAD_F, device=dev)
    d = torch.full((rows, c), PAD_F, device=dev)
    g = None if gout is None else torch.tensor([gout], dtype=torch.float32, device=dev)
    L.launch("pn2_weighted_ce_forward", tl, rows, c, L.ptr(tl), L.ptr(tlab), int(ldt == np.int64), L.ptr(tw), L.ptr(lse), L.ptr(acc), L.ptr(loss))
    L.launch("pn2_weighted_ce_backward", tl, rows, c, L.ptr(tl), L.ptr(tlab), int(ldt == np.int64), L.ptr(tw), L.ptr(lse), L.ptr(acc), L.ptr(g),
             L.ptr(d))
    return float(loss), lse.cpu().numpy(), d.cpu().numpy(), acc.cpu().numpy()


def ce_errors(ref, got, gout):
    """normalised errors (loss, lse, gradient) of a float32 result against the float64 reference"""
    loss64, lse64, grad64, loss_scale, grad_scale, _ = ref
    loss, lse, grad = got
    e_loss = abs(float(loss) - loss64) / loss_scale if np.isfinite(loss64) else (0.0 if float(loss) == loss64 else np.inf)
    e_lse = float(np.max(np.abs(lse.astype(np.float64) - lse64) / np.maximum(1.0, np.abs(lse64))))
    e_grad = float(np.max(np.abs(grad.astype(np.float64) - grad64 * float(np.float32(gout))) / (grad_scale * float(np.float32(gout)))))
    assert np.isfinite(grad).all() and np.isfinite(lse).all()
    return np.array([e_loss, e_lse, e_grad])


def ce_run_group(pn2, oracle, dev, cases, label_dtypes=(np.int32, np.int64)):
    """-> (worst float32-numpy errors, worst kernel errors) over `cases`, after asserting every kernel result is within 4 times
    the float32-numpy worst of the group"""
    refs = [ce_float64(oracle, *case) for case in cases]
    model = np.max([ce_errors(r, ce_float32(*case, GOUT), GOUT) for r, case in zip(refs, cases)], axis=0)
    bound = 4 * model
    worst = np.zeros(3)
    for r, case in zip(refs, cases):
        for ldt in label_dtypes:
            if ldt == np.int32 and ((case[1] < -2 ** 31) | (case[1] > 2 ** 31 - 1)).any():
                continue
            for gout in (GOUT, None):  # upstream scalar given / NULL (= 1)
                loss, lse, d, acc = ce_kernel(pn2._lib, dev, *case, ldt, gout)
                nzw = np.count_nonzero(np.where(r[5], case[2], 0))
                assert acc[1] == nzw, "non-zero-weight count %r, expected %d" % (acc[1], nzw)
                assert loss == r[0] or np.isfinite(r[0]), "loss %r, expected %r" % (loss, r[0])
                e = ce_errors(r, (loss, lse, d), 1.0 if gout is None else gout)
                worst = np.maximum(worst, e)
                assert (e <= bound).all(), "shape %s %s gout=%s: errors (loss, lse, grad) %s above 4 x float32 numpy %s" % (
                    case[0].shape, ldt.__name__, gout, e, model)
                assert (d[~r[5]] == 0).all(), "a row with an out-of-range label got a gradient"
    print("ce group: float32 numpy worst (loss, lse, grad) %s, kernel worst %s" % (model, worst))
    assert (worst > 0).any()
    return model, worst


@pytest.mark.parametrize("scale", CE_SCALES)
def test_weighted_ce_vs_float64_shape_grid(pn2, oracle, cuda, scale):
    """pn2_weighted_ce_forward / _backward by direct ABI calls (upstream scalar given and NULL, int32 and int64 labels) against
    oracle.weighted_sparse_ce and a float64 torch autograd, C in {1, 2, 9, 13, 64} x rows in {1, 255, 256, 257, 131072} and
    (16385, 64) whose rows * C passes the grid cap; logits scaled by 1, 30 and 1e4; a row of equal logits, a row with a -inf,
    weights 0 / denormal / negative / 1e6.  Loss, per-row lse and gradient must lie within 4 x the worst error of the same
    formula in float32 numpy over the same cases (per logit scale).  Errors are in units of: loss -- sum |w| max(1, |lse|,
    |z_label|) / nz; lse -- max(1, |lse|); gradient -- gout |w_r| / nz.

    Measured on an MI355X (loss, lse, gradient), float32 numpy worst / kernel worst:
      scale 1:   1.39e-07 2.16e-07 3.41e-07 / 1.39e-07 2.24e-07 3.39e-07
      scale 30:  6.46e-08 1.64e-07 3.99e-06 / 6.46e-08 1.64e-07 4.01e-06
      scale 1e4: 1.93e-07 5.74e-08 9.74e-04 / 1.93e-07 5.74e-08 9.74e-04  (lse ~ 3e4 is held to 2e-3, and p = exp(z - lse))"""
    cases = [ce_case(r, c, scale, 100 + i) for i, (r, c) in enumerate(CE_SHAPES)]
    ce_run_group(pn2, oracle, cuda, cases)


def test_weighted_ce_label_on_a_minus_inf_logit(pn2, oracle, cuda):
    """a row whose label sits on a -inf logit: the loss is +inf and is asserted as such; lse and the gradient stay finite and
    within the measured bound"""
    cases = [ce_case(r, c, 1.0, 300 + i, minus_inf_label=True) for i, (r, c) in enumerate([(8, 2), (257, 9), (131072, 13), (1000, 64)])]
    for case in cases:
        assert ce_float64(oracle, *case)[0] == np.inf
        assert ce_kernel(pn2._lib, cuda, *case, np.int64, None)[0] == np.inf
    ce_run_group(pn2, oracle, cuda, cases)


def test_weighted_ce_out_of_range_labels_act_as_weight_zero(pn2, oracle, cuda):
    """The contract of include/pn2_abi.h and model.get_loss: a row whose label is outside [0, C) behaves as weight 0 -- no
    loss, not counted in the non-zero denominator, zero gradient -- and forward and backward implement the same function: the
    gradient equals the float64 autograd gradient of that loss.  Labels -1 and C in both dtypes; as int64 also 2**31, -2**40
    and 2**32 + 3, whose low word is a valid class."""
    import torch
    out32 = lambda c: [-1, c, -2 ** 31, 2 ** 31 - 1, c + 1000]                      # noqa: E731
    out64 = lambda c: [-1, c, 2 ** 31, -2 ** 40, 2 ** 32 + 3, 2 ** 32, -2 ** 32 + 1]  # noqa: E731
    for ldt, outs in ((np.int32, out32), (np.int64, out64)):
        cases = []
        for i, (rows, c) in enumerate([(257, 9), (131072, 13), (1000, 64), (40, 4)]):
            logits, labels, w = ce_case(rows, c, 1.0, 400 + i)
            rs = np.random.RandomState(i)
            bad = np.flatnonzero(rs.random_sample(rows) < 0.2)
            labels[bad] = rs.choice(outs(c), bad.size)
            labels[8:8 + len(outs(c))] = outs(c)
            w[8:8 + len(outs(c))] = 1.0 + np.arange(len(outs(c)))  # weighty rows: a clamp to class 0 would show in the loss
            cases.append((logits, labels, w))
        model, _ = ce_run_group(pn2, oracle, cuda, cases, label_dtypes=(ldt,))
    # through the wrapper, whose docstring states the same contract
    logits, labels, w = cases[0]
    lt = torch.from_numpy(logits).to(cuda).requires_grad_(True)
    loss = pn2.model.get_loss(lt.reshape(1, *logits.shape), torch.from_numpy(labels).to(cuda).reshape(1, -1), torch.from_numpy(w).to(cuda).reshape(1, -1))
    (loss * GOUT).backward()
    ref = ce_float64(oracle, logits, labels, w)
    e = ce_errors(ref, (float(loss), ref[1].astype(np.float32), lt.grad.cpu().numpy()), GOUT)
    assert (e <= 4 * model).all(), (e, model)
    assert (lt.grad.cpu().numpy()[~ref[5]] == 0).all()
    # every label out of range: loss 0 (safe division), gradient 0
    labels[:] = -1
    loss, lse, d, acc = ce_kernel(pn2._lib, cuda, logits, labels, w, np.int64, GOUT)
    assert loss == 0.0 and (d == 0).all() and acc[1] == 0 and (np.abs(lse - ref[1]) / np.maximum(1, np.abs(ref[1]))).max() <= 4 * model[1]


# --------------------------------------------------------------------------------------------------------------------- Adam
ADAM_EDGES = np.array([0.0, 1e-20, -1e-20, 1e20, -1e20, 3e22, -3e22], np.float32)


def adam_f32_step(p, m, v, g, lr_t, b1, b2, eps, grad_scale):
    """adam_kernel's expressions in float32 numpy, in its order"""
    f = np.float32
    with np.errstate(all="ignore"):
        gi = g * f(grad_scale)
        m = f(b1) * m + (f(1) - f(b1)) * gi
        v = f(b2) * v + (f(1) - f(b2)) * gi * gi
        p = p - f(lr_t) * m / (np.sqrt(v) + f(eps))
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


@pytest.mark.parametrize("n", [1, 255, CAP * 2 + 3])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_adam_vs_float64_tf_formula(pn2, cuda, n, grad_scale):
    """pn2_adam_step against the float64 TF formula of test_adam_step_matches_tf_formula (adam_ref_step) with that test's
    tolerances, three steps, n = 1, 255 and 2 * 4096 * 256 + 3 (the grid-stride loop runs three times), grad_scale 1 and 1/8.
    Edge gradients, held over the steps, on parameters whose moments start at 0:
      g = 0: the parameter must not move (bit for bit);
      |g| = 1e-20: g * g underflows -- within the existing tolerances;
      |g| = 1e20: the kernel forms ((1 - beta2) g) g = 1e37, which float32 still holds, so it follows the float64 formula
        here (a step of about lr) rather than an overflowed g * g;
      |g| = 3e22: (1 - beta2) g g overflows to inf for both grad_scales: v = inf and the update is 0, not NaN -- the
        parameter stays bit for bit, m follows the formula.
    Tolerances: the existing test's.  They are relative to the RESULT, and b1 m + (1 - b1) g cancels when m and g have opposite
    signs (a few elements in 1e5; the existing test's draws happen to miss them), so an element may instead lie within 4 x the
    worst error of the same formula in float32 numpy (adam_f32_step, carried over the same steps), measured in units of the
    magnitudes that are added: |b1 m| + |(1 - b1) g| for m, b2 v + (1 - b2) g^2 for v, |p| + |update| for p.
    Measured on an MI355X: the kernel's p, m and v equal the float32 numpy evaluation bit for bit in every case and step
    here; worst float32 error in those units, n = 2097155, step 3: p 1.05e-6, m 5.09e-5 (a cancelled m of step 2 carried
    into step 3), v 2.66e-7."""
    import torch
    L = pn2._lib
    rs = np.random.RandomState(n % 97)
    p = rs.randn(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    k = min(n, len(ADAM_EDGES)) if n >= len(ADAM_EDGES) else 0
    tp, tm, tv = (torch.from_numpy(a.copy()).to(cuda) for a in (p, m, v))
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, 1e-3
    pr, mr, vr = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    fp, fm, fv = p.copy(), m.copy(), v.copy()
    ovf = np.zeros(n, bool)
    ovf[:k] = np.abs(ADAM_EDGES[:k]) > 1e21
    for t in range(1, 4):
        g = rs.randn(n).astype(np.float32) * (10.0 ** rs.randint(-3, 2))
        g[:k] = ADAM_EDGES[:k]
        lr_t = pn2.train.adam_lr_t(lr, t, b1, b2)
        hyper = torch.from_numpy(np.array([lr_t, b1, b2, eps, grad_scale], np.float32)).to(cuda)
        tg = torch.from_numpy(g).to(cuda)
        L.launch("pn2_adam_step", tp, n, L.ptr(tp), L.ptr(tg), L.ptr(tm), L.ptr(tv), L.ptr(hyper))
        f = np.float32
        ge = g.astype(np.float64) * float(f(grad_scale))
        sm = np.abs(float(f(b1)) * mr) + np.abs(float(f(1) - f(b1)) * ge)   # the magnitudes each sum adds, before the step
        sv = float(f(b2)) * vr + float(f(1) - f(b2)) * ge * ge
        p_before = pr
        pr, mr, vr = adam_ref_step(pr, mr, vr, g, lr_t, b1, b2, eps, grad_scale)
        sp = np.abs(p_before) + np.abs(pr - p_before)
        fp, fm, fv = adam_f32_step(fp, fm, fv, g, lr_t, b1, b2, eps, grad_scale)
        gp, gm, gv = tp.cpu().numpy(), tm.cpu().numpy(), tv.cpu().numpy()
        assert np.array_equal(bits(tg.cpu().numpy()), bits(g))
        for name, got, mod, ref, scale, rtol, atol, sel in (("p", gp, fp, pr, sp, 2e-6, 2e-7, ~ovf), ("m", gm, fm, mr, sm, 2e-6, 1e-9, ovf | ~ovf),
                                                            ("v", gv, fv, vr, sv, 2e-6, 1e-12, ~ovf)):
            scale = np.maximum(scale[sel], 1e-30)
            e32 = float(np.max(np.abs(mod[sel].astype(np.float64) - ref[sel]) / scale))
            err = np.abs(got[sel].astype(np.float64) - ref[sel])
            tol = np.maximum(atol + rtol * np.abs(ref[sel]), 4 * e32 * scale)
            print("adam n=%d gs=%g t=%d %s: float32 numpy worst %.3g, kernel worst %.3g, bit-equal to float32 numpy: %s" % (
                n, grad_scale, t, name, e32, float(np.max(err / scale)), np.array_equal(bits(got[sel]), bits(mod[sel]))))
            assert (err <= tol).all(), "%s: %d elements off, worst %.3g x its tolerance" % (name, (err > tol).sum(), (err / tol).max())
        if k:
            assert bits(gp[:1]) == bits(p[:1]) and gm[0] == 0 and gv[0] == 0          # g = 0: nothing moves
            assert np.isinf(gv[ovf]).all() and np.array_equal(bits(gp[ovf]), bits(p[ovf]))  # v = inf: update 0, not NaN
            assert np.isfinite(gp).all() and np.isfinite(gm).all()
            assert abs(abs(gp[3] - p[3]) - t * lr) < 0.2 * t * lr                      # |g| = 1e20 still steps by about lr


def test_adam_single_edge_elements(pn2, cuda):
    """n = 1 with each edge gradient in turn (m = v = 0, one step)"""
    import torch
    L = pn2._lib
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, 1e-3
    lr_t = pn2.train.adam_lr_t(lr, 1, b1, b2)
    for gs in (1.0, 0.125):
        hyper = torch.from_numpy(np.array([lr_t, b1, b2, eps, gs], np.float32)).to(cuda)
        for g in ADAM_EDGES:
            tp, tm, tv = (torch.tensor([a], dtype=torch.float32, device=cuda) for a in (0.75, 0.0, 0.0))
            tg = torch.tensor([g], dtype=torch.float32, device=cuda)
            L.launch("pn2_adam_step", tp, 1, L.ptr(tp), L.ptr(tg), L.ptr(tm), L.ptr(tv), L.ptr(hyper))
            pr, mr, vr = adam_ref_step(np.array([0.75]), np.zeros(1), np.zeros(1), np.array([g], np.float32), lr_t, b1, b2, eps, gs)
            np.testing.assert_allclose(tm.cpu().numpy(), mr, rtol=2e-6, atol=1e-9)
            if abs(g) > 1e21:
                assert np.isinf(float(tv)) and float(tp) == 0.75
            else:
                np.testing.assert_allclose(tp.cpu().numpy(), pr, rtol=2e-6, atol=2e-7)
                np.testing.assert_allclose(tv.cpu().numpy(), vr, rtol=2e-6, atol=1e-12)
            if g == 0:
                assert float(tp) == 0.75 and float(tm) == 0 and float(tv) == 0


# --------------------------------------------------------------------------------------------------------------- multi copy
def test_multi_copy_fill_direct(pn2, cuda):
    """pn2_multi_copy_fill by direct ABI calls, byte for byte: 0 to 4 fills of mixed 4 and 8 bytes (a 4-byte fill ignores the high
    half of its value and leaves the four bytes after its target alone), copy lists with zero-byte entries, an all-zero-byte
    list, 48 entries, sources and destinations 1 to 3 bytes (and 4, 8 bytes) off a 16-byte boundary."""
    import ctypes
    import torch
    L = pn2._lib
    rs = np.random.RandomState(2)
    fills = [(0, 8, 0x1122334455667788), (8, 4, 0xDEADBEEF12345678), (20, 4, 0xFFFFFFFF00000001), (24, 8, 0x8000000000000001)]
    sizes48 = [0, 1, 15, 16, 17, 4099, 0, 3, 64, 70001, 5, 1000003] * 4
    for sizes, nfill in [(sizes48, 4), (sizes48, 0), (sizes48[:5], 1), ([0, 0, 0], 2), ([0], 3), ([33], 4), ([0, 7, 0], 0)]:
        srcs, dsts, exps, ptrs_s, ptrs_d = [], [], [], [], []
        for i, nb in enumerate(sizes):
            so, do = 16 + (i * 7) % 16, 16 + (i * 5 + 1) % 16
            if i % 6 == 3:
                so = do = 16  # both aligned: the 16-byte path with a byte tail
            s_np = rs.randint(0, 256, nb + 48).astype(np.uint8)
            srcs.append(torch.from_numpy(s_np).to(cuda))
            dsts.append(torch.full((nb + 48,), PAD_B, dtype=torch.uint8, device=cuda))
            e = np.full(nb + 48, PAD_B, np.uint8)
            e[do:do + nb] = s_np[so:so + nb]
            exps.append(e)
            ptrs_s.append(srcs[-1].data_ptr() + so)
            ptrs_d.append(dsts[-1].data_ptr() + do)
        n = len(sizes)
        fbuf = torch.full((48,), 0xEE, dtype=torch.uint8, device=cuda)
        fexp = np.full(48, 0xEE, np.uint8)
        for off, nb, val in fills[:nfill]:
            fexp[off:off + nb] = np.frombuffer(int(val).to_bytes(8, "little")[:nb], np.uint8)
        args = (n, (ctypes.c_void_p * n)(*ptrs_s), (ctypes.c_void_p * n)(*ptrs_d), L.u64_array(sizes), nfill,
                (ctypes.c_void_p * max(nfill, 1))(*[fbuf.data_ptr() + f[0] for f in fills[:nfill]]) if nfill else None,
                L.u64_array([f[2] for f in fills[:nfill]]) if nfill else None, L.int_array([f[1] for f in fills[:nfill]]) if nfill else None)
        L.launch("pn2_multi_copy_fill", fbuf, *args)
        for i in range(n):
            assert np.array_equal(dsts[i].cpu().numpy(), exps[i]), (sizes[i], i, nfill)
        assert np.array_equal(fbuf.cpu().numpy(), fexp), nfill


# ------------------------------------------------------------------------------------------------------------ group pooling
FAR = 19.0  # exp(-5 * 19) = 5.5e-42: a float32 denormal


def pool_case(rows, k, c, seed):
    """x with exact ties in the max (row 0: the same value at 2 neighbours, row 1: at all k) and neighbour offsets with row 2 at
    distance 0, row 3 one near / the others far (denormal weights next to a weight of 1), row 4 all far (every weight denormal)"""
    rs = np.random.RandomState(seed)
    x = rs.randn(rows, k, c).astype(np.float32)
    g = (rs.randn(rows, k, 3) * 0.3).astype(np.float32)
    far = np.zeros(rows, bool)
    if rows >= 5:
        x[0, -1] = x[0, 0] = np.abs(x[0]).max(axis=0) + 1
        x[1, :] = x[1, 0]
        g[2] = 0.0
        g[3] = [FAR, 0, 0]
        g[3, 0] = 0.0
        g[4] = np.array([0, FAR, 0], np.float32) + g[4] * 0.01
        far[4] = True
    return x, g, rs.randn(rows, c).astype(np.float32), rs.randn(rows, 2 * c).astype(np.float32), far


def pool_ref(x, g, dout, mode, dt):
    """forward and gradient in dtype `dt`, neighbours summed in order (float64: the reference; float32: the kernel's formula)"""
    rows, k, c = x.shape
    x = x.astype(dt)
    with np.errstate(all="ignore"):
        if mode == 2:
            gg = g.astype(dt)
            e = np.exp(-np.sqrt((gg[..., 0] * gg[..., 0] + gg[..., 1] * gg[..., 1]) + gg[..., 2] * gg[..., 2]) * dt(5))
            ws = np.zeros(rows, dt)
            for j in range(k):
                ws = ws + e[:, j]
            w = e / ws[:, None]
        else:
            w = np.full((rows, k), dt(1) / dt(k), dt)
        mx = x.max(axis=1)
        tie = x == mx[:, None, :]
        ties = tie.sum(axis=1).astype(dt)
        sm = np.zeros((rows, c), dt)
        for j in range(k):
            sm = sm + x[:, j] * (w[:, j, None] if mode == 2 else dt(1))
        avg = sm if mode == 2 else sm / dt(k)
        d = dout.astype(dt)
        if mode == 0:
            return mx, np.where(tie, (d / ties)[:, None, :], dt(0))
        if mode in (1, 2):
            return avg, d[:, None, :] * w[:, :, None] + np.zeros_like(x)
        return np.concatenate([avg, mx], 1), d[:, None, :c] * w[:, :, None] + np.where(tie, (d[:, c:] / ties)[:, None, :], dt(0))


def pool_kernel(L, dev, x, g, dout, mode, off=0):
    import torch
    rows, k, c = x.shape
    oc = 2 * c if mode == 3 else c
    vx, vo, vd = View(dev, x.size, torch.float32, off, x.reshape(-1)), View(dev, rows * oc, torch.float32), View(dev, x.size, torch.float32, off)
    tg = torch.from_numpy(g).to(dev) if mode == 2 else None
    td = torch.from_numpy(np.ascontiguousarray(dout)).to(dev)
    L.launch("pn2_group_pool", vx.t, rows, k, c, mode, vx.ptr(), L.ptr(tg), vo.ptr())
    L.launch("pn2_group_pool_grad", vx.t, rows, k, c, mode, vx.ptr(), L.ptr(tg), L.ptr(td), vd.ptr())
    assert np.array_equal(bits(vx.get()), bits(x.reshape(-1)))
    return vo.get().reshape(rows, oc), vd.get().reshape(rows, k, c)


def pool_errors(x, dout, far, ref, got):
    """normalised by max_j |x_j| (forward) and |dout| (gradient); -> worst (forward, gradient) over ordinary rows and over rows
    whose weights are all denormal"""
    c = x.shape[2]
    xs = np.maximum(np.abs(x).max(axis=1).astype(np.float64), 1e-30)
    xs = np.concatenate([xs] * (ref[0].shape[1] // c), 1)
    ds = np.abs(dout.astype(np.float64))
    ds = np.maximum(ds[:, :c] + (ds[:, c:] if ref[0].shape[1] > c else 0), 1e-30)
    with np.errstate(all="ignore"):
        ef = (np.abs(got[0].astype(np.float64) - ref[0]) / xs).max(axis=1)
        eg = (np.abs(got[1].astype(np.float64) - ref[1]) / ds[:, None, :]).max(axis=(1, 2))
    ef, eg = np.where(np.isnan(ef), np.inf, ef), np.where(np.isnan(eg), np.inf, eg)
    grp = lambda e, sel: float(e[sel].max()) if sel.any() else 0.0  # noqa: E731
    return np.array([grp(ef, ~far), grp(eg, ~far), grp(ef, far), grp(eg, far)])


POOL_SHAPES = [(7, k, c, 0) for c in (1, 3, 4, 36, 130) for k in (1, 2, 32)] + [(7, 32, 4, 1), (9, 2, 36, 3), (CAP + 1, 2, 4, 0)]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_group_pool_and_gradient_vs_float64(pn2, cuda, mode):
    """pn2_group_pool / pn2_group_pool_grad, modes max, avg, weighted_avg and max_and_avg, against float64 numpy: c in {1, 3, 4,
    36, 130} x k in {1, 2, 32}, x one and three elements off a 16-byte boundary, and 4096 * 256 + 1 rows (both kernels' grids
    are capped).  Exact ties in the max -- the same value at 2 and at all k neighbours -- split the gradient evenly, as
    tf.reduce_max does.  weighted_avg with neighbours at distance 0 and at 19, where exp(-5 d) = 5.5e-42 is denormal; rows whose
    weights are ALL denormal carry only ~12 bits and are measured as a group of their own.  Bound: 4 x the worst error of the
    same formula in float32 numpy over the same cases, in units of max_j |x_j| (forward) and |dout| (gradient).

    Measured on an MI355X, (forward, gradient) float32 numpy worst / kernel worst -- ordinary rows; all-denormal rows:
      max:          0 0 / 0 0;  0 0 / 0 0   (exact)
      avg:          4.98e-07 0 / 4.98e-07 0;  5.46e-08 0 / 5.46e-08 0
      weighted_avg: 4.52e-07 2.85e-07 / 4.52e-07 2.85e-07;  4.73e-05 2.83e-05 / 4.73e-05 2.83e-05
      max_and_avg:  4.98e-07 5.91e-08 / 4.98e-07 5.91e-08;  5.46e-08 5.88e-08 / 5.46e-08 5.88e-08
    (the kernel's worst equals the float32 numpy worst in every mode)"""
    L = pn2._lib
    cases = [pool_case(r, k, c, 500 + i) + (off,) for i, (r, k, c, off) in enumerate(POOL_SHAPES)]
    dout = lambda cs: cs[3] if mode == 3 else cs[2]  # noqa: E731
    refs = [pool_ref(cs[0], cs[1], dout(cs), mode, np.float64) for cs in cases]
    model = np.max([pool_errors(cs[0], dout(cs), cs[4], r, pool_ref(cs[0], cs[1], dout(cs), mode, np.float32)) for cs, r in zip(cases, refs)], axis=0)
    worst = np.zeros(4)
    for cs, r in zip(cases, refs):
        x, g, _, _, far, off = cs
        out, dx = pool_kernel(L, cuda, x, g, dout(cs), mode, off)
        e = pool_errors(x, dout(cs), far, r, (out, dx))
        worst = np.maximum(worst, e)
        assert (e <= 4 * model).all(), "mode %d shape %s off %d: errors %s above 4 x float32 numpy %s" % (mode, x.shape, off, e, model)
        c = x.shape[2]
        if mode in (0, 3):  # the max itself is exact, and so is the even split of a tie
            assert np.array_equal(bits(out[:, -c:]), bits(x.max(axis=1)))
        if mode == 0 and x.shape[0] >= 5:
            k = x.shape[1]
            d = dout(cs)
            assert np.array_equal(bits(dx[1]), bits(np.broadcast_to(d[1] / np.float32(k), (k, c))))           # all k tie: g / k each
            if k > 2:
                assert np.array_equal(bits(dx[0, 0]), bits(d[0] / np.float32(2))) and np.array_equal(bits(dx[0, -1]), bits(dx[0, 0]))
                assert (dx[0, 1:-1] == 0).all()                                                                # 2 tie: g / 2 each
    print("pool mode %d: float32 numpy worst %s, kernel worst %s" % (mode, model, worst))
