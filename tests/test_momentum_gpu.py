"""pn2_momentum_step (csrc/pn2_train.hip) against tf.train.MomentumOptimizer's formula in float64 (use_nesterov = False, reference
train.py:380-383):  g' = g * grad_scale;  accum <- momentum * accum + g';  p <- p - lr * accum.

Sizes on both sides of the 16-byte vector, of one block and of the 4096-block grid cap; views that start off a 16-byte boundary
(the whole call then takes the scalar path) bit-equal to the aligned run (vector path + scalar tail); the edge gradients and
coefficients; the gradient buffer left as it was.  Where float32 is held against float64 the tolerances are those of
test_train_gpu.test_adam_step_matches_tf_formula, with the cancellation clause of test_train_tail_gpu
.test_adam_vs_float64_tf_formula: momentum * accum + g' cancels when the two have opposite signs, so an element may instead
lie within 4 x the worst error of the same expressions in float32 numpy, in units of the magnitudes that are added."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 4096 * 256  # grid_1d: at most 4096 blocks of 256 threads, then grid-stride
P_RTOL, P_ATOL, A_RTOL, A_ATOL = 2e-6, 2e-7, 2e-6, 1e-9  # test_adam_step_matches_tf_formula's, for p and for the first moment
EDGES = np.array([0.0, 1e20, -1e20], np.float32)
SENTINEL = 7.25


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def momentum_ref_step(p, a, g, lr, mom, grad_scale):
    """one step in float64 on float64 state (p, accum) with the float32 gradient g -> (p, accum).  The kernel holds lr, momentum
    and grad_scale as float32 (as adam_ref_step has it for Adam)."""
    f = np.float32
    ge = np.asarray(g, f).astype(np.float64) * float(f(grad_scale))
    a = float(f(mom)) * a + ge
    return p - float(f(lr)) * a, a


def momentum_f32_step(p, a, g, lr, mom, grad_scale):
    """momentum_kernel's expressions in float32 numpy, in its order"""
    f = np.float32
    with np.errstate(all="ignore"):
        gi = g * f(grad_scale)
        a = f(mom) * a + gi
        p = p - f(lr) * a
    assert p.dtype == a.dtype == f
    return p, a


class View:
    """n floats inside a larger tensor, `off` floats past a 16-byte boundary, the floats around them filled with a sentinel"""

    def __init__(self, dev, data, off):
        import torch
        n = data.size
        self.lead, self.n = 4 + off, n
        self.base = torch.full((self.lead + n + 8,), SENTINEL, dtype=torch.float32, device=dev)
        assert self.base.data_ptr() % 16 == 0
        self.t = self.base[self.lead:self.lead + n]
        assert self.t.data_ptr() % 16 == 4 * off
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32)))

    def get(self):
        b = self.base.cpu().numpy()
        assert (b[:self.lead] == SENTINEL).all() and (b[self.lead + self.n:] == SENTINEL).all(), "wrote outside its view"
        return b[self.lead:self.lead + self.n].copy()


def launch(L, n, tp, tg, ta, hyper):
    L.launch("pn2_momentum_step", tp, n, L.ptr(tp), L.ptr(tg), L.ptr(ta), L.ptr(hyper))


def check_against_float64(tag, got_p, got_a, f32_p, f32_a, ref_p, ref_a, scale_p, scale_a):
    """tolerance per element: the project's rtol / atol on the result, or 4 x the float32 evaluation's worst error in units of the
    magnitudes added; prints whether the kernel equals the float32 numpy evaluation bit for bit (not asserted: a compiler may
    contract the multiply-add)"""
    for name, got, mod, ref, scale, rtol, atol in (("p", got_p, f32_p, ref_p, scale_p, P_RTOL, P_ATOL),
                                                   ("accum", got_a, f32_a, ref_a, scale_a, A_RTOL, A_ATOL)):
        scale = np.maximum(scale, 1e-30)
        e32 = float(np.max(np.abs(mod.astype(np.float64) - ref) / scale))
        err = np.abs(got.astype(np.float64) - ref)
        tol = np.maximum(atol + rtol * np.abs(ref), 4 * e32 * scale)
        print("momentum %s %s: float32 numpy worst %.3g, kernel worst %.3g, bit-equal to float32 numpy: %s" % (
            tag, name, e32, float(np.max(err / scale)), np.array_equal(bits(got), bits(mod))))
        assert (err <= tol).all(), "%s %s: %d elements off, worst %.3g x its tolerance" % (tag, name, (err > tol).sum(),
                                                                                          (err / tol).max())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 257, 2 * CAP + 3])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_momentum_vs_float64_tf_formula(pn2, cuda, n, grad_scale):
    """three consecutive steps with a new gradient each (accum is carried), one element up to three passes of the grid-stride loop.
    From n = 3 on the first elements hold the edge gradients over all steps, on accum = 0: g = 0 moves nothing (bit for bit),
    |g| = 1e20 at lr = 1e-3 stays finite and follows the formula.  The gradient buffer is bit for bit what was uploaded."""
    import torch
    L = pn2._lib
    rs = np.random.RandomState(n % 97)
    p = rs.randn(n).astype(np.float32)
    k = len(EDGES) if n >= len(EDGES) else 0
    tp, ta = torch.from_numpy(p.copy()).to(cuda), torch.zeros(n, dtype=torch.float32, device=cuda)
    lr, mom = 1e-3, 0.9
    hyper = torch.from_numpy(np.array([lr, mom, grad_scale], np.float32)).to(cuda)
    pr, ar = p.astype(np.float64), np.zeros(n)
    fp, fa = p.copy(), np.zeros(n, np.float32)
    f = np.float32
    for t in range(1, 4):
        g = rs.randn(n).astype(np.float32) * f(10.0 ** rs.randint(-3, 2))
        g[:k] = EDGES[:k]
        tg = torch.from_numpy(g).to(cuda)
        launch(L, n, tp, tg, ta, hyper)
        ge = g.astype(np.float64) * float(f(grad_scale))
        scale_a = np.abs(float(f(mom)) * ar) + np.abs(ge)  # the magnitudes each sum adds, before the step
        p_before = pr
        pr, ar = momentum_ref_step(pr, ar, g, lr, mom, grad_scale)
        scale_p = np.abs(p_before) + np.abs(float(f(lr)) * ar)
        fp, fa = momentum_f32_step(fp, fa, g, lr, mom, grad_scale)
        gp, ga = tp.cpu().numpy(), ta.cpu().numpy()
        assert np.array_equal(bits(tg.cpu().numpy()), bits(g)), "the gradient buffer was written"
        check_against_float64("n=%d gs=%g t=%d" % (n, grad_scale, t), gp, ga, fp, fa, pr, ar, scale_p, scale_a)
        assert np.isfinite(gp).all() and np.isfinite(ga).all()
        if k:
            assert bits(gp[:1]) == bits(p[:1]) and bits(ga[:1]) == bits(np.zeros(1, f))  # g = 0: nothing moves
            assert ga[1] > 1e19 * grad_scale and ga[2] < -1e19 * grad_scale and gp[1] < -1e15 and gp[2] > 1e15


def test_momentum_single_edge_elements(pn2, cuda):
    """n = 1 with each edge gradient in turn (accum = 0), three steps of the same gradient"""
    import torch
    L = pn2._lib
    lr, mom = 1e-3, 0.9
    for gs in (1.0, 0.125):
        hyper = torch.from_numpy(np.array([lr, mom, gs], np.float32)).to(cuda)
        for g in EDGES:
            tp, ta = (torch.tensor([v], dtype=torch.float32, device=cuda) for v in (0.75, 0.0))
            tg = torch.tensor([g], dtype=torch.float32, device=cuda)
            pr, ar = np.array([0.75]), np.zeros(1)
            for _ in range(3):
                launch(L, 1, tp, tg, ta, hyper)
                pr, ar = momentum_ref_step(pr, ar, np.array([g], np.float32), lr, mom, gs)
                np.testing.assert_allclose(tp.cpu().numpy(), pr, rtol=P_RTOL, atol=P_ATOL)
                np.testing.assert_allclose(ta.cpu().numpy(), ar, rtol=A_RTOL, atol=A_ATOL)
            assert np.isfinite(float(tp)) and np.isfinite(float(ta))
            if g == 0:
                assert bits(tp.cpu().numpy()) == bits(np.float32(0.75)) and bits(ta.cpu().numpy()) == bits(np.float32(0.0))
            assert float(tg) == g


def test_momentum_zero_coefficients(pn2, cuda):
    """momentum = 0: accum is g' bit for bit (every step forgets the one before);  lr = 0: the parameters stay bit for bit while
    accum follows the formula.  n = 1031: vector body and a three-element scalar tail."""
    import torch
    L = pn2._lib
    n = 1031
    f = np.float32
    for gs in (1.0, 0.125):
        rs = np.random.RandomState(11)
        p = rs.randn(n).astype(np.float32)
        # momentum = 0
        tp, ta = torch.from_numpy(p.copy()).to(cuda), torch.zeros(n, dtype=torch.float32, device=cuda)
        hyper = torch.from_numpy(np.array([1e-3, 0.0, gs], np.float32)).to(cuda)
        pr = p.astype(np.float64)
        for t in range(3):
            g = rs.randn(n).astype(np.float32) * f(10.0 ** rs.randint(-3, 2))
            launch(L, n, tp, torch.from_numpy(g).to(cuda), ta, hyper)
            assert np.array_equal(bits(ta.cpu().numpy()), bits(g * f(gs))), "momentum 0, step %d" % t
            pr, _ = momentum_ref_step(pr, np.zeros(n), g, 1e-3, 0.0, gs)
            np.testing.assert_allclose(tp.cpu().numpy(), pr, rtol=P_RTOL, atol=P_ATOL)
        # lr = 0
        tp, ta = torch.from_numpy(p.copy()).to(cuda), torch.zeros(n, dtype=torch.float32, device=cuda)
        hyper = torch.from_numpy(np.array([0.0, 0.9, gs], np.float32)).to(cuda)
        pr, ar = p.astype(np.float64), np.zeros(n)
        fp, fa = p.copy(), np.zeros(n, f)
        for t in range(3):
            g = rs.randn(n).astype(np.float32) * f(10.0 ** rs.randint(-3, 2))
            launch(L, n, tp, torch.from_numpy(g).to(cuda), ta, hyper)
            ge = g.astype(np.float64) * float(f(gs))
            scale_a = np.abs(float(f(0.9)) * ar) + np.abs(ge)
            pr, ar = momentum_ref_step(pr, ar, g, 0.0, 0.9, gs)
            fp, fa = momentum_f32_step(fp, fa, g, 0.0, 0.9, gs)
            assert np.array_equal(bits(tp.cpu().numpy()), bits(p)), "lr 0, step %d: a parameter moved" % t
            check_against_float64("lr=0 gs=%g t=%d" % (gs, t), tp.cpu().numpy(), ta.cpu().numpy(), fp, fa, pr, ar,
                                  np.abs(pr), scale_a)


def test_momentum_result_does_not_depend_on_alignment(pn2, cuda):
    """The same 1031 values on tensors as torch allocates them (16-byte aligned: 257 vectors + 3 scalar elements), then on views
    that start 1, 2 and 3 floats into a larger allocation -- params, grads and accum shifted one at a time, then all together:
    each such call runs entirely on the scalar path.  Three steps each; p and accum are bit-equal to the aligned run, and the
    floats in front of and behind every view keep their sentinel."""
    import torch
    L = pn2._lib
    n = 1031
    rs = np.random.RandomState(5)
    p0 = rs.randn(n).astype(np.float32)
    gs_ = [rs.randn(n).astype(np.float32) * np.float32(10.0 ** e) for e in (0, -2, 1)]
    hyper = torch.from_numpy(np.array([1e-3, 0.9, 0.125], np.float32)).to(cuda)
    tp, ta = torch.from_numpy(p0.copy()).to(cuda), torch.zeros(n, dtype=torch.float32, device=cuda)
    want = []
    for g in gs_:
        tg = torch.from_numpy(g).to(cuda)
        assert tp.data_ptr() % 16 == 0 and tg.data_ptr() % 16 == 0 and ta.data_ptr() % 16 == 0
        launch(L, n, tp, tg, ta, hyper)
        want.append((tp.cpu().numpy().copy(), ta.cpu().numpy().copy()))
    assert not np.array_equal(want[0][0], p0)
    for off in (1, 2, 3):
        for shifted in ((off, 0, 0), (0, off, 0), (0, 0, off), (off, off, off)):
            vp, va = View(cuda, p0, shifted[0]), View(cuda, np.zeros(n, np.float32), shifted[2])
            for t, g in enumerate(gs_):
                vg = View(cuda, g, shifted[1])
                launch(L, n, vp.t, vg.t, va.t, hyper)
                assert np.array_equal(bits(vg.get()), bits(g)), (shifted, t)
                assert np.array_equal(bits(vp.get()), bits(want[t][0])), (shifted, t)
                assert np.array_equal(bits(va.get()), bits(want[t][1])), (shifted, t)


def test_momentum_step_direct_abi_return_codes(pn2, cuda):
    """the raw entry point on the device: 0 for a good call, and a refused call leaves the buffers alone"""
    import torch
    L = pn2._lib
    tp = torch.ones(8, dtype=torch.float32, device=cuda)
    tg, ta = torch.ones_like(tp), torch.zeros_like(tp)
    hyper = torch.tensor([0.5, 0.0, 1.0], dtype=torch.float32, device=cuda)
    assert L.lib.pn2_momentum_step(0, L.ptr(tp), L.ptr(tg), L.ptr(ta), L.ptr(hyper), L.stream_ptr()) == -1
    assert L.lib.pn2_momentum_step(8, L.ptr(tp), None, L.ptr(ta), L.ptr(hyper), L.stream_ptr()) == -2
    assert float(tp.sum()) == 8.0 and float(ta.sum()) == 0.0
    assert L.lib.pn2_momentum_step(8, L.ptr(tp), L.ptr(tg), L.ptr(ta), L.ptr(hyper), L.stream_ptr()) == 0
    assert torch.equal(tp, torch.full_like(tp, 0.5)) and torch.equal(ta, torch.ones_like(ta))
    assert isinstance(L.ptr(tp), ctypes.c_void_p)
