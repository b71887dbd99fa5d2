"""GPU tests of the training path of pointnet_sa_module_msg on the hoisted library kernels: pn2_sa_hoist_rows_multi_bn against the
one-scale entry point and float64 statistics, pn2_scatter_plan_apply_multi against pn2_scatter_plan_apply, the module (geometry
computed ahead by msg_geometry) against a float64 restatement in plain torch, its capture into one graph, and the fall-backs.

Shapes: b=2, n=257, m=19, C=16, scales K=(3, 16, 40[, 1]) with first-layer widths (4, 32, 68[, 8]): odd sizes, several workgroups
per scale, 1 / 8 / 17 float4 columns (17 does not divide the workgroup), a smallest radius that leaves centroids with a single hit
(rows padded with the repeated first index), full groups at the largest.  m=70 is added for the module test: from 2048 rows per
layer on, the layers of a stack hand over un-normalised outputs (tf_util.can_defer_bn), and the hoisted first layer then
publishes its batch norm's constants itself."""
import types

import numpy as np
import pytest

from test_layers_gpu import T

pytestmark = pytest.mark.gpu

B, N, C = 2, 257, 16
RADII, KS, WIDTHS = (0.12, 0.3, 2.0, 0.2), (3, 16, 40, 1), (4, 32, 68, 8)
MLPS = [[4, 8], [32, 32, 64], [68]]
POISON, PAD = -7.25, 64


@pytest.fixture(scope="module")
def S(pn2, cuda):
    """inputs and geometry shared by the tests of this file (computed once, never modified)"""
    import torch
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    keep = tfu.get_default_store()
    rs = np.random.RandomState(20260)
    s = types.SimpleNamespace()
    s.xyz = T(rs.rand(B, N, 3).astype(np.float32), cuda)
    s.pts = T(rs.randn(B, N, C).astype(np.float32), cuda)
    s.geo = {m: pu.msg_geometry(s.xyz, m, RADII, KS) for m in (19, 70)}
    cnts = [c for _, c in pn2.tf_ops.tf_grouping.query_ball_point_multi(RADII, KS, s.xyz, s.geo[19][0])]
    assert bool((cnts[0] == 1).any()), "the smallest radius leaves some centroids with a single hit"
    assert bool((cnts[2] >= KS[2]).all()), "every group is full at the largest radius"
    idx0 = s.geo[19][1][0]
    assert bool((idx0[cnts[0] == 1] == idx0[cnts[0] == 1][:, :1]).all())  # ... whose row repeats the first index
    torch.cuda.synchronize()
    yield s
    tfu.set_default_store(keep)
    tfu.USE_HOISTED_MSG_TRAIN = True


def _guarded(shape, dev, dtype=None, fill=None):
    """a tensor of `shape` inside a larger buffer of POISON -> (buffer, view)"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), POISON, dtype=dtype or torch.float32, device=dev)
    v = buf[PAD:PAD + n]
    if fill is not None:
        v.fill_(fill)
    return buf, v.view(shape)


def _intact(buf):
    return bool((buf[:PAD] == POISON).all()) and bool((buf[-PAD:] == POISON).all())


def _geo(S, m, nsc):
    new_xyz, idxs, plans = S.geo[m]
    return new_xyz, idxs[:nsc], plans[:nsc]


# ---- 1. the kernel against the one-scale entry point ----------------------------------------------------------------------------
@pytest.mark.parametrize("nsc", [1, 3, 4])
@pytest.mark.parametrize("finish", [1, 2])
def test_hoist_multi_equals_the_single_scale_kernel_and_float64_statistics(pn2, cuda, S, nsc, finish):
    import torch
    L = pn2._lib
    tfu = pn2.util.tf_util
    m = 19
    new_xyz, idxs, _ = _geo(S, m, nsc)
    rs = np.random.RandomState(100 + nsc)
    couts, ks = WIDTHS[:nsc], KS[:nsc]
    # z: the scales' column blocks with unused (NaN) columns between and behind them
    gaps = (0, 4, 0, 8)
    zcols, col = [], 0
    for s in range(nsc):
        col += gaps[s]
        zcols.append(col)
        col += couts[s]
    z_stride = col + 4
    z = torch.full((B * N, z_stride), float("nan"), device=cuda)
    for s in range(nsc):
        z[:, zcols[s]:zcols[s] + couts[s]] = T((rs.randn(B * N, couts[s]) + 3.0 * rs.randn(couts[s])).astype(np.float32), cuda)
    wx = [T(rs.randn(3, c).astype(np.float32), cuda) for c in couts]
    gamma = [T((1 + 0.2 * rs.randn(c)).astype(np.float32), cuda) for c in couts]
    beta = [T((0.1 * rs.randn(c)).astype(np.float32), cuda) for c in couts]
    bias = [T((0.05 * rs.randn(c)).astype(np.float32), cuda) for c in couts]
    yb, gb, wsb, smb, sib, scb, shb, rmb, rvb = ([] for _ in range(9))
    for s in range(nsc):
        rows = B * m * ks[s]
        yb.append(_guarded((rows, couts[s]), cuda))
        gb.append(_guarded((rows, 3), cuda))
        wsb.append(_guarded((L.lib.pn2_bn_workspace_bytes(couts[s]) // 8,), cuda, torch.float64, fill=0.0))
        for lst, fill in ((smb, None), (sib, None), (scb, None), (shb, None), (rmb, 0.0), (rvb, 1.0)):
            lst.append(_guarded((couts[s],), cuda, fill=fill))
    view = lambda lst: [v for _, v in lst]  # noqa: E731
    two = finish == 2
    L.launch("pn2_sa_hoist_rows_multi_bn", z, nsc, B, N, m, z_stride, L.ptr(S.xyz), L.ptr(new_xyz), L.ptr(z), L.int_array(ks),
             L.int_array(couts), L.int_array(zcols), L.ptr_table(idxs), L.ptr_table(wx), L.ptr_table(view(yb)), L.ptr_table(view(gb)),
             L.ptr_table(view(wsb)), L.u64_array([L.nbytes(v) for v in view(wsb)]), L.int_array([finish] * nsc),
             L.ptr_table(gamma) if two else None, L.ptr_table(beta) if two else None, L.ptr_table(bias) if two else None, 1e-3, 0.5,
             L.ptr_table(view(rmb)) if two else None, L.ptr_table(view(rvb)) if two else None,
             L.ptr_table(view(smb)) if two else None, L.ptr_table(view(sib)) if two else None,
             L.ptr_table(view(scb)) if two else None, L.ptr_table(view(shb)) if two else None)
    torch.cuda.synchronize()
    for s in range(nsc):
        rows, c = B * m * ks[s], couts[s]
        y, g = yb[s][1], gb[s][1]
        assert not bool(torch.isnan(y).any()), "an unused column of z reached y"
        zs = z[:, zcols[s]:zcols[s] + c].contiguous()
        y1, g1 = torch.empty_like(y), torch.empty_like(g)
        L.launch("pn2_sa_hoist_rows", zs, B, N, m, ks[s], c, L.ptr(S.xyz), L.ptr(new_xyz), L.ptr(idxs[s]), L.ptr(zs), L.ptr(wx[s]),
                 L.ptr(y1), L.ptr(g1))
        assert torch.equal(y, y1) and torch.equal(g, g1), "scale %d" % s
        for lst in (yb, gb, wsb) + ((smb, sib, scb, shb, rmb, rvb) if two else ()):
            assert _intact(lst[s][0]), "scale %d: a write outside an output" % s
        if not two:  # finish 1: the folded sums are in the workspace; the project's normalisation kernel turns them into moments
            rm, rv = torch.zeros(c, device=cuda), torch.ones(c, device=cuda)
            _, _, sm, si = tfu._bn_train_forward(y, bias[s], gamma[s], beta[s], rm, rv, 0.5, True, 0, (wsb[s][1], L.BN_WS_FOLDED))
            sc = sh = None
        else:
            sm, si, sc, sh, rm, rv = (lst[s][1] for lst in (smb, sib, scb, shb, rmb, rvb))
        yd = y.double().cpu().numpy()
        mean, var = yd.mean(0), yd.var(0)
        invstd = 1.0 / np.sqrt(var + 1e-3)
        ga, be, bi = (t[s].cpu().numpy() for t in (gamma, beta, bias))
        # the tolerances of test_train_gpu.py::test_deferred_batch_norm_constants_and_load_transform_vs_float64 for the same quantities
        np.testing.assert_allclose(sm.cpu().numpy(), mean, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(si.cpu().numpy(), invstd, rtol=1e-5)
        if two:
            np.testing.assert_allclose(sc.cpu().numpy(), ga * invstd, rtol=2e-5, atol=1e-7)
            np.testing.assert_allclose(sh.cpu().numpy(), be - mean * ga * invstd, rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(rm.cpu().numpy(), 0.5 * (mean + bi), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rv.cpu().numpy(), 0.5 + 0.5 * var * rows / (rows - 1), rtol=1e-5)


# ---- 2. the scatter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsc", [1, 3, 4])
def test_scatter_apply_multi_equals_the_single_plan_kernel(pn2, cuda, S, nsc):
    import torch
    L = pn2._lib
    pu = pn2.util.pointnet_util
    m = 19
    _, idxs, plans = _geo(S, m, nsc)
    rs = np.random.RandomState(200 + nsc)
    couts, ks = WIDTHS[:nsc], KS[:nsc]
    # (first column, width) of the slice of a wider gradient each plan reads: dense / 12 bytes off a 16-byte boundary (the
    # 4-byte-aligned loads) / a 16-byte aligned slice of a wider row / dense
    slices = ((0, couts[0]),) + ((3, 3 + WIDTHS[1]), (4, WIDTHS[2] + 8), (0, WIDTHS[3]))[:nsc - 1]
    wide = [T(rs.randn(B, m * ks[s], slices[s][1]).astype(np.float32), cuda) for s in range(nsc)]
    ocols, col = [], 4
    for s in range(nsc):
        ocols.append(col)
        col += couts[s] + (8 if s == 1 else 0)
    out_stride = col + 4
    buf, out = _guarded((B, N, out_stride), cuda, fill=float("nan"))
    L.launch("pn2_scatter_plan_apply_multi", out, nsc, B, N, out_stride, L.int_array([m * k for k in ks]), L.int_array([1] * nsc),
             L.int_array(couts), L.int_array(ocols), (L.c_void_p * nsc)(*[wide[s].data_ptr() + 4 * slices[s][0] for s in range(nsc)]),
             L.int_array([sl[1] for sl in slices]), L.ptr_table(plans), L.u64_array([p.numel() for p in plans]), L.ptr(out))
    torch.cuda.synchronize()
    assert _intact(buf)
    covered = torch.zeros(out_stride, dtype=torch.bool, device=cuda)
    for s in range(nsc):
        one = pu._scatter_plan_apply(plans[s], wide[s], slices[s][0], couts[s], m * ks[s], 1, N)
        assert torch.equal(out[:, :, ocols[s]:ocols[s] + couts[s]], one), "scale %d" % s
        covered[ocols[s]:ocols[s] + couts[s]] = True
    assert bool(torch.isnan(out[:, :, ~covered]).all()) and int((~covered).sum()) >= 8


# ---- 3. the module against float64 ----------------------------------------------------------------------------------------------
_OWN = object()


def _fresh_store(pn2, cuda, S, m, mlps, ks, radii, seed=11, pts=_OWN, **kw):
    """a store holding the module's variables with non-trivial gamma / beta / biases"""
    import torch
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    store = tfu.set_default_store(tfu.VariableStore(device=cuda, seed=seed))
    with torch.no_grad():
        pu.pointnet_sa_module_msg(S.xyz, S.pts if pts is _OWN else pts, m, radii, ks, mlps, True, 0.5, "msg", **kw)  # creates the variables
        g = torch.Generator().manual_seed(seed)
        for k, p in store.params.items():
            if k.endswith("gamma"):
                p.copy_((1 + 0.2 * torch.randn(p.shape, generator=g)).to(cuda))
            elif k.endswith("beta") or k.endswith("biases"):
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(cuda))
    return store


def _reset_buffers(store):
    for k, v in store.buffers.items():
        v.fill_(1.0 if k.endswith("moving_variance") else 0.0)


def _run_module(pn2, S, store, m, geometry, flag, pts, dy):
    import torch
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    tfu.set_default_store(store)
    tfu.reset_bn_links()
    _reset_buffers(store)
    for p in store.parameters():
        p.grad = None
    calls = []
    orig = tfu.conv2d_hoisted_first_msg
    tfu.conv2d_hoisted_first_msg = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    tfu.USE_HOISTED_MSG_TRAIN = flag
    try:
        x = pts.clone().requires_grad_(True)
        new_xyz, out = pu.pointnet_sa_module_msg(S.xyz, x, m, RADII[:3], KS[:3], MLPS, True, 0.5, "msg", geometry=geometry)
        out.backward(dy)
        torch.cuda.synchronize()
    finally:
        tfu.USE_HOISTED_MSG_TRAIN = True
        tfu.conv2d_hoisted_first_msg = orig
    assert len(calls) == (1 if flag else 0)
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in store.params.items()}
    return out.detach(), x.grad.detach().clone(), grads, {k: v.clone() for k, v in store.buffers.items()}


def _restatement(store, xyz, pts, new_xyz, idxs, mlps, dy):
    """the module in float64, plain torch: gather, concat [features | xyz], train_layer_torch per layer, max over K"""
    import torch
    from torch_layers import train_layer_torch
    p64 = {k: p.detach().double().requires_grad_(True) for k, p in store.params.items()}
    buf = {k: (torch.ones_like(v) if k.endswith("moving_variance") else torch.zeros_like(v)).double() for k, v in store.buffers.items()}
    x = pts.detach().double().requires_grad_(True)
    xyz, new_xyz = xyz.double(), new_xyz.double()
    bi = torch.arange(xyz.shape[0], device=xyz.device)[:, None, None]
    outs = []
    for s, idx in enumerate(idxs):
        gi = idx.long()
        h = torch.cat([x[bi, gi], xyz[bi, gi] - new_xyz[:, :, None, :]], dim=-1)
        for j, cout in enumerate(mlps[s]):
            sc = "msg/conv%d_%d/" % (s, j)
            bnv = (p64[sc + "bn/beta"], p64[sc + "bn/gamma"], buf[sc + "bn/moving_mean"], buf[sc + "bn/moving_variance"])
            h = train_layer_torch(h, p64[sc + "weights"].reshape(-1, cout), p64[sc + "biases"], bnv, 0.5, True)
        outs.append(h.amax(dim=2))
    out = torch.cat(outs, dim=-1)
    out.backward(dy.double())
    return out.detach(), x.grad, {k: p.grad for k, p in p64.items()}, buf


def _check_against(got, ref, what):
    out, dpts, grads, bufs = got
    rout, rdpts, rgrads, rbufs = ref
    # a batch-normed layer's output: the project's figure (test_train_gpu.py:64)
    np.testing.assert_allclose(out.cpu().numpy(), rout.cpu().numpy(), rtol=1e-4, atol=2e-5, err_msg=what)
    # every gradient within 1e-4 of the tensor's largest entry: the project's whole-model gradient bound
    worst = {}
    for k, r in list(rgrads.items()) + [("points", rdpts)]:
        g = dpts if k == "points" else grads[k]
        if g is None:  # a bias in front of batch norm: the HIP layers return no gradient, it is exactly zero
            assert k.endswith("biases") and float(r.abs().max()) < 1e-6, k
            continue
        worst[k] = float((g.double() - r).abs().max()) / float(r.abs().max())
    print(what, "gradient errors relative to the tensor's max:", {k: "%.1e" % v for k, v in worst.items()})
    assert len(worst) >= 1 + 3 * 6 and max(worst.values()) <= 1e-4, (what, max(worst, key=worst.get), max(worst.values()))
    # the moving averages moved once, to the restatement's values: the figures of a layer's moving averages
    # (test_train_gpu.py:62-63; the looser of the two for both, the deeper layers' inputs carry fp32 rounding)
    for k, r in rbufs.items():
        np.testing.assert_allclose(bufs[k].cpu().numpy(), r.cpu().numpy(), rtol=2e-5, atol=1e-6, err_msg=what + " " + k)


@pytest.mark.parametrize("m", [19, 70])
def test_module_training_path_against_float64(pn2, cuda, S, m):
    """figures on an MI355X are printed by _check_against (run with -s)"""
    import torch
    geo = _geo(S, m, 3)
    store = _fresh_store(pn2, cuda, S, m, MLPS, KS[:3], RADII[:3])
    dy = T(np.random.RandomState(300 + m).randn(B, m, sum(mlp[-1] for mlp in MLPS)).astype(np.float32), cuda)
    ref = _restatement(store, S.xyz, S.pts, geo[0], geo[1], MLPS, dy)
    hoisted = _run_module(pn2, S, store, m, geo, True, S.pts, dy)
    assert hoisted[0].shape == (B, m, 8 + 64 + 68) and hoisted[0].dtype == torch.float32
    _check_against(hoisted, ref, "hoisted m=%d" % m)
    # the same comparison on the existing path: the restatement, not the new path, is the yardstick
    _check_against(_run_module(pn2, S, store, m, geo, False, S.pts, dy), ref, "flag off m=%d" % m)


# ---- 4. the geometry ------------------------------------------------------------------------------------------------------------
def test_msg_geometry_is_what_the_module_computes(pn2, cuda, S):
    import torch
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    m = 19
    new_xyz, idxs, plans = S.geo[m]
    seen = []
    orig = pu.query_ball_point_multi
    pu.query_ball_point_multi = lambda *a, **k: (seen.append(orig(*a, **k)), seen[-1])[1]
    try:
        tfu.set_default_store(tfu.VariableStore(device=cuda, seed=1))
        with torch.no_grad():
            own_xyz, _ = pu.pointnet_sa_module_msg(S.xyz, S.pts, m, RADII, KS, [[8]] * 4, True, 0.5, "msg")
    finally:
        pu.query_ball_point_multi = orig
    assert len(seen) == 1 and len(idxs) == 4 and len(plans) == 4
    assert torch.equal(new_xyz, own_xyz)
    for s in range(4):
        assert idxs[s].dtype == torch.int32 and torch.equal(idxs[s], seen[0][s][0])
    assert pu.msg_geometry(S.xyz, m, RADII, KS, plans=False)[2] == [None] * 4
    rs = np.random.RandomState(400)
    for s in range(4):
        dy = rs.randn(B, m * KS[s], 8).astype(np.float32)
        got = pu._scatter_plan_apply(plans[s], T(dy, cuda), 0, 8, m * KS[s], 1, N).cpu().numpy()
        ref = np.zeros((B, N, 8))
        ii = idxs[s].cpu().numpy().reshape(B, -1)
        for b in range(B):
            np.add.at(ref[b], ii[b], dy[b].astype(np.float64))
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------
def test_module_forward_backward_in_one_captured_graph(pn2, cuda, S):
    import torch
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    m = 19
    geo = _geo(S, m, 3)
    store = _fresh_store(pn2, cuda, S, m, MLPS, KS[:3], RADII[:3])
    rs = np.random.RandomState(500)
    width = sum(mlp[-1] for mlp in MLPS)
    batches = [(T(rs.randn(B, N, C).astype(np.float32), cuda), T(rs.randn(B, m, width).astype(np.float32), cuda)) for _ in range(3)]
    eager = [_run_module(pn2, S, store, m, geo, True, p, d) for p, d in batches]
    x = batches[0][0].clone().requires_grad_(True)
    dy = batches[0][1].clone()
    for p in store.parameters():
        p.grad = None
    tfu.reset_bn_links()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one capture stream; the module opens no side stream
        _, out = pu.pointnet_sa_module_msg(S.xyz, x, m, RADII[:3], KS[:3], MLPS, True, 0.5, "msg", geometry=geo)
        out.backward(dy)
    for (p, d), ref in list(zip(batches, eager))[1:]:  # replayed twice on refilled static inputs
        with torch.no_grad():
            x.copy_(p)
            dy.copy_(d)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref[0].cpu().numpy(), rtol=1e-4, atol=2e-5)
        for k, r in list(ref[2].items()) + [("points", ref[1])]:
            g = x.grad if k == "points" else store.params[k].grad
            if r is None:
                assert g is None, k
                continue
            assert float((g - r).abs().max()) <= 1e-4 * float(r.abs().max()), k


# ---- 6. the fall-backs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["five_scales", "no_points", "no_xyz", "narrow_points"])
def test_fall_backs_use_the_given_geometry_on_the_existing_path(pn2, cuda, S, case):
    import torch
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    m = 19
    radii, ks, mlps = list(RADII[:3]), list(KS[:3]), [[8], [32, 16], [12]]
    pts, kw = S.pts, {}
    if case == "five_scales":
        radii, ks, mlps = list(RADII) + [0.5], list(KS) + [8], mlps + [[8], [16]]
    elif case == "no_points":
        pts = None
    elif case == "no_xyz":
        kw = dict(use_xyz=False)
    else:
        pts = S.pts[:, :, :8].contiguous()
    geo = pu.msg_geometry(S.xyz, m, radii, ks)

    def refuse(*a, **k):
        raise AssertionError("the hoisted path was taken")

    orig = tfu.conv2d_hoisted_first_msg
    tfu.conv2d_hoisted_first_msg = refuse
    try:
        res = []
        for g in (geo, None):
            store = _fresh_store(pn2, cuda, S, m, mlps, ks, radii, pts=pts, **kw)
            _reset_buffers(store)
            tfu.reset_bn_links()
            x = None if pts is None else pts.clone().requires_grad_(True)
            new_xyz, out = pu.pointnet_sa_module_msg(S.xyz, x, m, radii, ks, mlps, True, 0.5, "msg", geometry=g, **kw)
            out.sum().backward()
            res.append((new_xyz, out.detach(), None if x is None else x.grad))
    finally:
        tfu.conv2d_hoisted_first_msg = orig
    assert torch.equal(res[0][0], res[1][0]) and res[0][0] is geo[0]
    # the same kernels on the same inputs; the batch statistics are sums of fp64 atomics, whose order may move the last bit of a mean
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)
    if pts is not None:  # ... and the order inside the scatter lists of the grouping's gradient is arbitrary (fp32 sums of <= 40 terms)
        assert float((res[0][2] - res[1][2]).abs().max()) <= 1e-5 * float(res[1][2].abs().max())
