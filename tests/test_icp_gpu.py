"""GPU tests of rigid registration: pn2_icp and pn2_transform_points (csrc/pn2_icp.hip) against the numpy model of the rules
(tests/icp_ref.py); every output between poisoned guards, every input compared unchanged, the workspace poisoned; pn2.icp's
wrappers, the KITTI method and examples/register_frames.py.

There is no tolerance anywhere: a partner is decided by float64 comparisons, the sums are float64 in one fixed tree over the
source index, and everything after them is float64 in a fixed association without contraction, with correctly rounded sqrt and
division.  correspondence, header, result and trace are compared with the model bit for bit.  Nothing here captures a graph.

The model is brute force (an ns x nt pair matrix per evaluation), so a case has a few hundred points.  Where a case is about the
grid, the clouds are laid out by CELL (edge r * (1 + 2^-20), counted from the TARGET's minimum) and the expected partners are
known by construction as well."""
import ctypes
import importlib.util
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_ref as R  # noqa: E402
from icp_cases import TRUTH, corner, corner_bound, moved_corner, rigid  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5
G = 64       # guard bytes in front of and behind every output
F = np.float64


def _guarded(torch, dev, nbytes):
    raw = torch.full((G + nbytes + G,), POISON, dtype=torch.uint8, device=dev)
    return raw, raw[G:G + nbytes]


def _payload(raw, nbytes, what):
    h = raw.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[G + nbytes:] == POISON).all(), "%s: written outside its bounds" % what
    return h[G:G + nbytes]


def _matrix(T):
    return None if T is None else (ctypes.c_double * 16)(*np.asarray(T, dtype=F).reshape(-1))


def _run(pn2, dev, src, tgt, r, est=0, init=None, max_iteration=0, tol=(1e-6, 1e-6), slab=None, tlab=None, nrm=None, trace=True):
    """pn2_icp -> icp_ref.Result (trace None when not asked for): every output inside its guards, the inputs unchanged, nothing
    written behind the workspace"""
    import torch
    lib = pn2._lib
    ns, nt = len(src), len(tgt)
    host = dict(src=src, tgt=tgt, slab=slab, tlab=tlab, nrm=nrm)
    d = {k: None if v is None else torch.from_numpy(v).to(dev) for k, v in host.items()}
    sizes = dict(correspondence=4 * ns, result=160, trace=160 * (max_iteration + 1), header=32)
    raw, out = {}, {}
    for name, nbytes in sizes.items():
        raw[name], out[name] = (None, None) if name == "trace" and not trace else _guarded(torch, dev, nbytes)
    nbytes = ctypes.c_ulonglong(0)
    lib.launch("pn2_icp_workspace_size", dev, ns, nt, max_iteration, ctypes.byref(nbytes), stream=False)
    ws = torch.full((int(nbytes.value) + 255 + G,), POISON, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    lib.launch("pn2_icp", dev, ns, lib.ptr(d["src"]), lib.ptr(d["slab"]), nt, lib.ptr(d["tgt"]), lib.ptr(d["tlab"]), lib.ptr(d["nrm"]),
               float(np.float32(r)), est, _matrix(init), max_iteration, float(tol[0]), float(tol[1]), lib.ptr(out["correspondence"]),
               lib.ptr(out["result"]), lib.ptr(out["trace"]), lib.ptr(out["header"]), ws.data_ptr() + off, int(nbytes.value))
    torch.cuda.synchronize()
    for k, v in host.items():
        assert v is None or d[k].cpu().numpy().tobytes() == v.tobytes(), "%s changed" % k
    assert (ws[off + int(nbytes.value):] == POISON).all(), "written behind the workspace"
    got = {name: None if raw[name] is None else _payload(raw[name], nbytes, name) for name, nbytes in sizes.items()}
    return R.Result(got["correspondence"].view(np.int32), got["result"].view(F),
                    None if got["trace"] is None else got["trace"].view(F).reshape(max_iteration + 1, 20), got["header"].view(np.int32))


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(len(got), -1), want.reshape(len(want), -1)
        rows = np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(g, w)])[0]
        raise AssertionError("%s: rows %s\n%r\n%r" % (what, rows[:8], g[rows[:3]], w[rows[:3]]))


def _check(pn2, dev, src, tgt, r, est=0, init=None, max_iteration=0, tol=(1e-6, 1e-6), slab=None, tlab=None, nrm=None):
    """the library against the model, bit for bit -> the model's Result"""
    src = np.ascontiguousarray(src, dtype=np.float32)
    tgt = np.ascontiguousarray(tgt, dtype=np.float32)
    slab = None if slab is None else np.ascontiguousarray(slab, dtype=np.int32)
    tlab = None if tlab is None else np.ascontiguousarray(tlab, dtype=np.int32)
    nrm = None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float32)
    got = _run(pn2, dev, src, tgt, r, est, init, max_iteration, tol, slab, tlab, nrm)
    want = R.icp(src, tgt, r, est, init, max_iteration, tol[0], tol[1], slab, tlab, nrm)
    assert got.header.tolist() == want.header.tolist()
    assert got.correspondence.tolist() == want.correspondence.tolist()
    _same_bits(got.result, want.result, "result")
    _same_bits(got.trace, want.trace, "trace")
    return want


def _pair_of_clouds(seed, ns, nt, noise=0.01):
    """a corner of nt points with its normals as the target; ns of its points, drawn with repetition, moved by about a degree and
    0.05 units and jittered, as the source"""
    rs = np.random.RandomState(seed)
    tgt, nrm = corner(seed, nt)
    inv = np.linalg.inv(rigid([1, -1, 2], 1.0, [0.03, 0.02, -0.03]))
    pick = tgt[rs.randint(0, nt, ns)].astype(F) + rs.normal(0, noise, (ns, 3))
    return (pick @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32), tgt, nrm


# ---- sizes: partial waves, one / two / three rows of partials ----------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 255, 256, 257, 513])
def test_source_sizes(pn2, cuda, ns):
    src, tgt, nrm = _pair_of_clouds(ns, ns, 150)
    for est in (0, 1):
        want = _check(pn2, cuda, src, tgt, 0.4, est, max_iteration=3, nrm=nrm)
        assert want.header[1] == ns and want.header[3] >= min(ns, 3)


@pytest.mark.parametrize("nt", [1, 2, 64, 65])
def test_target_sizes(pn2, cuda, nt):
    src, tgt, nrm = _pair_of_clouds(100 + nt, 100, nt)
    for est in (0, 1):
        want = _check(pn2, cuda, src, tgt, 0.4, est, max_iteration=2, nrm=nrm)
        assert want.header[2] == nt and want.header[3] > 0


# ---- the grid -----------------------------------------------------------------------------------------------------------------
def test_partners_in_every_neighbouring_cell(pn2, cuda):
    """r = 1.  Source j = 0 .. 26 sits in the middle of cell (2 + 5 j, 2, 2) and its only target within reach 0.55 away along
    the offset j of {-1, 0, 1}^3: in that neighbouring cell (the own cell for the offset 0), at most 0.953 away.  Source 27 and
    its target are 1.1 apart with a cell between them: strangers."""
    offsets = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3)
    src = np.array([[2.5 + 5 * j, 2.5, 2.5] for j in range(27)] + [[2.5, 7.95, 2.5]])
    tgt = np.concatenate([[[0.0, 0.0, 0.0]], src[:27] + 0.55 * offsets, [[2.5, 9.05, 2.5]]])
    order = np.random.RandomState(0).permutation(len(tgt))  # (the target index is not the sorted position)
    tgt = tgt[order]
    where = np.argsort(order)
    want = _check(pn2, cuda, src, tgt, 1.0)
    assert want.correspondence.tolist() == [where[1 + j] for j in range(27)] + [-1] and want.header[3] == 27
    cells = np.floor(tgt[want.correspondence[:27]].astype(np.float32).astype(F) / (1.0 + 2.0 ** -20)).astype(int)
    assert np.array_equal(cells - [[2 + 5 * j, 2, 2] for j in range(27)], offsets)
    _check(pn2, cuda, src, tgt, 1.0, max_iteration=2)


def test_source_points_outside_the_targets_grid(pn2, cuda):
    """r = 1, the target's box is [0, 3.2]^3: source points in cell -1 (partner in cell 0), in cell -2 (none), one cell beyond
    the top cell (partner in the top cell), two beyond (none), on every axis; and so far out that the cell coordinate leaves
    [-1, 2^21] and the int range altogether"""
    tgt = np.array([[0, 0, 0], [3.2, 3.2, 3.2], [0.2, 0, 0], [0, 3.2, 0], [3.2, 0, 3.2], [1.5, 1.5, 1.5]])
    src, want = [], []
    for a in range(3):
        e = np.eye(3)[a]
        src += [-0.5 * e, -1.5 * e, np.array([3.2, 3.2, 3.2]) + 0.9 * e, np.array([3.2, 3.2, 3.2]) + 2.0 * e]
        want += [0, -1, 1, -1]
    src += [[1e30, 0, 0], [0, -1e30, 0], [0, 0, 3e38], [2.2e6, 0, 0], [-3.0, -3.0, -3.0], [1.4, 1.6, 1.5]]
    want += [-1, -1, -1, -1, -1, 5]
    out = _check(pn2, cuda, np.array(src), tgt, 1.0)
    assert out.correspondence.tolist() == want and out.header.tolist() == [0, len(src), 6, 7, 0, 0, 0, 0]


def test_ties_and_duplicates(pn2, cuda):
    """two targets at exactly the same distance in different cells -- the one the scan meets first has the higher index --, and
    duplicated target rows: the lowest index wins"""
    tgt = np.array([[0, 0, 0], [9, 9, 9], [9, 9, 9], [0.5, 0.5, 0.5], [4.5, 4.5, 4.5], [4.5, 4.5, 4.5], [1.5, 0.5, 0.5], [4.5, 4.5, 4.5]])
    tgt = tgt[[0, 1, 2, 6, 4, 5, 3, 7]]  # index 3 = (1.5, .5, .5) in cell x = 1, index 6 = (.5, .5, .5) in cell x = 0
    src = np.array([[1.0, 0.5, 0.5], [4.5, 4.25, 4.5], [9, 9, 9.5]])
    want = _check(pn2, cuda, src, tgt, 1.0)
    assert want.correspondence.tolist() == [3, 4, 1] and want.result[18] == 0.25 + 0.0625 + 0.25
    _check(pn2, cuda, src, tgt[::-1], 1.0)


def test_the_boundary_is_inclusive(pn2, cuda):
    tgt = np.array([[3, 4, 0], [0, 0, -5], [20, 20, 20]], dtype=np.float32)
    src = np.array([[0, 0, 0], [20, 20, 25]], dtype=np.float32)
    assert _check(pn2, cuda, src, tgt, 5.0).correspondence.tolist() == [0, 2]  # distance exactly 5: in
    below = np.nextafter(np.float32(5.0), np.float32(0.0))
    assert _check(pn2, cuda, src, tgt, below).correspondence.tolist() == [-1, -1]  # one float32 step less: out


# ---- invalid rows -------------------------------------------------------------------------------------------------------------
def test_invalid_rows(pn2, cuda):
    rs = np.random.RandomState(4)
    src, tgt, nrm = _pair_of_clouds(4, 300, 200)
    slab, tlab = rs.randint(0, 3, 300), rs.randint(0, 3, 200)
    slab[rs.choice(300, 30, replace=False)] = -1 - rs.randint(0, 4, 30)
    tlab[rs.choice(200, 20, replace=False)] = [-1, -2 ** 31] * 10
    bad = rs.choice(300, 9, replace=False)
    src[bad[:3], 0], src[bad[3:6], 1], src[bad[6:], 2] = np.nan, np.inf, -np.inf
    bad = rs.choice(200, 9, replace=False)
    tgt[bad[:3], 2], tgt[bad[3:6], 0], tgt[bad[6:], 1] = np.nan, -np.inf, np.inf
    nbad = rs.choice(200, 12, replace=False)
    nrm[nbad[:4], 0], nrm[nbad[4:8], 1], nrm[nbad[8:], 2] = np.nan, np.inf, -np.inf
    s_ok = R.valid_mask(src, slab)
    for est in (0, 1):
        want = _check(pn2, cuda, src, tgt, 0.4, est, max_iteration=3, slab=slab, tlab=tlab, nrm=nrm)
        t_ok = R.valid_mask(tgt, tlab, nrm if est else None)
        assert want.header[1] == s_ok.sum() and want.header[2] == t_ok.sum() and want.header[3] > 100
        assert (want.correspondence[~s_ok] == -1).all() and t_ok[want.correspondence[want.correspondence >= 0]].all()
    # the normals decide validity for point-to-plane only
    assert R.valid_mask(tgt, tlab, nrm).sum() < R.valid_mask(tgt, tlab).sum()
    # labels on one side only
    _check(pn2, cuda, src, tgt, 0.4, 0, max_iteration=1, slab=slab)
    _check(pn2, cuda, src, tgt, 0.4, 1, max_iteration=1, tlab=tlab, nrm=nrm)


def test_overflow_and_nothing_valid(pn2, cuda):
    src, tgt, nrm = _pair_of_clouds(5, 70, 80)
    src[7] = [3e38, 0, 0]
    src[8] = [-2e38, 1, 1]
    init = np.diag([2.0, 1.0, 1.0, 1.0])  # 6e38 and -4e38 are not float32s: inf, no partner; the others still match
    init[0, 3] = -3.0
    want = _check(pn2, cuda, src, tgt, 3.0, init=init, max_iteration=1)
    assert want.correspondence[7] == -1 and want.correspondence[8] == -1 and want.header[1] == 70 and want.header[3] > 0
    assert np.isinf(R.transform_rows(src, init)[[7, 8], 0]).all()
    # an all-invalid source: m = 0, fitness 0, rmse 0, status 2 at the first update
    for est in (0, 1):
        want = _check(pn2, cuda, src, tgt, 0.4, est, max_iteration=2, slab=np.full(70, -1), nrm=nrm)
        assert want.header.tolist() == [2, 0, 80, 0, 0, 0, 0, 0] and want.result[16:].tolist() == [0, 0, 0, 0]
        want = _check(pn2, cuda, src, tgt, 0.4, est, max_iteration=0, slab=np.full(70, -1), nrm=nrm)
        assert want.header.tolist() == [0, 0, 80, 0, 0, 0, 0, 0]
    # an all-invalid target: nobody has a partner
    want = _check(pn2, cuda, src[:9], tgt, 0.4, max_iteration=1, tlab=np.full(80, -3))
    assert want.header.tolist() == [2, 7 + 2, 0, 0, 0, 0, 0, 0] and (want.correspondence == -1).all()


# ---- the loop -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iteration", [0, 1, 8])
def test_iteration_counts(pn2, cuda, max_iteration):
    src, tgt, nrm = moved_corner()
    for est in (0, 1):
        want = _check(pn2, cuda, src, tgt, 0.5, est, max_iteration=max_iteration, tol=(0.0, 0.0), nrm=nrm)
        # a tolerance of 0 never stops the loop: every update is applied
        assert want.header[0] == 0 and want.header[4] == max_iteration and want.header[5] == 0
        if max_iteration == 0:
            assert np.array_equal(want.result[:16].reshape(4, 4), np.eye(4)) and want.result[17] > 0.05


@pytest.mark.parametrize("est,k", [(0, 5), (1, 4)])
def test_the_criterion_stops_the_loop_early(pn2, cuda, est, k):
    """moved_corner() converges at evaluation k (5 point-to-point, 4 point-to-plane: tests/test_icp_cpu.py) of 12: the launches
    behind it find `done` and write nothing -- T, the header and the correspondence are those of evaluation k, the trace rows
    behind it stay zero.  And the model's final pose is within the CPU file's measured bound of the truth."""
    src, tgt, nrm = moved_corner()
    want = _check(pn2, cuda, src, tgt, 0.5, est, max_iteration=12, nrm=nrm)
    assert want.header.tolist() == [0, 400, 400, 400, k, 1, 0, 0] and (want.trace[k + 1:] == 0).all() and (want.trace[k, 4:] != 0).any()
    assert np.array_equal(want.trace[k, 4:], want.result[:16]) and want.correspondence.tolist() == list(range(400))
    assert np.abs(want.result[:16].reshape(4, 4) - TRUTH).max() <= corner_bound()
    # one round fewer than it needs: the same T_k, not converged
    short = _check(pn2, cuda, src, tgt, 0.5, est, max_iteration=k, nrm=nrm)
    assert short.header[4] == k and np.array_equal(short.result[:16], want.result[:16])


def test_too_few_pairs_and_parallel_normals(pn2, cuda):
    tgt, nrm = corner(6, 60)
    far = np.array([50.0, 50.0, 50.0])

    def source(m):  # m points with a partner, 5 without
        return np.concatenate([tgt[:m].astype(F) + 0.01, far + np.arange(15).reshape(5, 3)])

    for est, few in ((0, 2), (1, 5)):
        want = _check(pn2, cuda, source(few), tgt, 0.2, est, max_iteration=4, nrm=nrm)
        assert want.header.tolist() == [2, few + 5, 60, few, 0, 0, 0, 0] and np.array_equal(want.result[:16].reshape(4, 4), np.eye(4))
        assert want.result[16] == few / (few + 5.0) and want.result[17] > 0
        want = _check(pn2, cuda, source(few + 1), tgt, 0.2, est, max_iteration=4, nrm=nrm)
        assert want.header[3] >= few + 1 and (want.header[0] == 0 or est == 1)  # (six pairs may still leave a pivot at zero)
        assert _check(pn2, cuda, source(few), tgt, 0.2, est, max_iteration=0, nrm=nrm).header[0] == 0  # evaluation only: fine
    # all normals parallel: the in-plane motion is free, a pivot is not positive
    src, tgt, nrm = moved_corner()
    flat = np.zeros_like(nrm)
    flat[:, 2] = 1
    want = _check(pn2, cuda, src, tgt, 0.5, 1, max_iteration=4, nrm=flat)
    assert want.header[0] == 2 and want.header[3] == 400 and want.header[4] == 0


def test_status_1_for_a_target_too_wide_for_the_grid(pn2, cuda):
    src, tgt, nrm = _pair_of_clouds(7, 70, 90)
    tgt[17, 1] = -3e6
    init = rigid([0, 0, 1], 30.0, [1, 2, 3])
    for est in (0, 1):
        want = _check(pn2, cuda, src, tgt, 1.0, est, init=init, max_iteration=3, nrm=nrm)
        assert want.header.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and (want.correspondence == -1).all()
        assert np.array_equal(want.result[:16].reshape(4, 4), init) and (want.result[16:] == 0).all() and (want.trace[1:] == 0).all()
    tgt[17, 1] = -1.5e6  # 1.5 * 10^6 cells: still fine
    assert _check(pn2, cuda, src, tgt, 1.0, 0, max_iteration=1).header[0] == 0


def test_init_and_trace_are_optional(pn2, cuda):
    src, tgt, nrm = _pair_of_clouds(8, 257, 120)
    src, tgt = np.ascontiguousarray(src), np.ascontiguousarray(tgt)
    for est in (0, 1):
        given = _run(pn2, cuda, src, tgt, 0.4, est, np.eye(4), 3, nrm=nrm)
        for init, trace in ((None, True), (np.eye(4), False), (None, False)):
            other = _run(pn2, cuda, src, tgt, 0.4, est, init, 3, nrm=nrm, trace=trace)
            assert (other.trace is None) == (not trace)
            for name in ("correspondence", "result", "header") + (("trace",) if trace else ()):
                assert getattr(other, name).tobytes() == getattr(given, name).tobytes(), name
    # an init that does the work: the source under a 30 degree turn, handed back by init
    turn = rigid([0, 0, 1], 30.0, [0.5, -0.25, 0.125])
    inv = np.linalg.inv(turn)
    turned = (src.astype(F) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    want = _check(pn2, cuda, turned, tgt, 0.4, 0, init=turn, max_iteration=3)
    assert want.trace[0, 1] > 0.9 and _check(pn2, cuda, turned, tgt, 0.4, 0, max_iteration=0).result[16] < 0.5
    _check(pn2, cuda, turned, tgt, 0.4, 1, init=turn, max_iteration=3, nrm=nrm)


# ---- the transform ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_transform_points(pn2, cuda, n):
    import torch
    lib = pn2._lib
    rs = np.random.RandomState(n)
    pts = (rs.uniform(-50, 50, (n, 3))).astype(np.float32)
    if n > 10:
        pts[3], pts[5], pts[7], pts[9] = [np.nan, 1, 2], [1, np.inf, 2], [1, 2, -np.inf], [3e38, -3e38, 1]
    T = rigid([1, 1, -2], 40.0, [5, -6, 7])
    T[0, 0] *= 1.5  # (any finite matrix)
    d_pts = torch.from_numpy(pts).to(cuda)
    raw, out = _guarded(torch, cuda, 12 * n)
    lib.launch("pn2_transform_points", cuda, n, lib.ptr(d_pts), _matrix(T), lib.ptr(out))
    torch.cuda.synchronize()
    assert d_pts.cpu().numpy().tobytes() == pts.tobytes()
    want = R.transform_points(pts, T)
    assert _payload(raw, 12 * n, "out").tobytes() == want.tobytes()
    lib.launch("pn2_transform_points", cuda, n, lib.ptr(d_pts), _matrix(T), lib.ptr(d_pts))  # in place
    assert d_pts.cpu().numpy().tobytes() == want.tobytes()


# ---- refusals that need a device -----------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing(pn2, cuda):
    import torch
    lib = pn2._lib
    n = 100
    pts = torch.zeros((n, 3), dtype=torch.float32, device=cuda)
    outs = [_guarded(torch, cuda, b) for b in (4 * n, 160, 160 * 3, 32)]
    (corr, res, trace, hdr) = [o[1] for o in outs]
    nbytes = ctypes.c_ulonglong(0)
    lib.launch("pn2_icp_workspace_size", cuda, n, n, 2, ctypes.byref(nbytes), stream=False)
    need = int(nbytes.value)
    ws = torch.full((need + 512,), POISON, dtype=torch.uint8, device=cuda)
    off = (-ws.data_ptr()) % 256

    def call(n=n, r=0.5, est=0, init=None, it=2, tol=1e-6, workspace=ws.data_ptr() + off, nbytes=need, corr=corr, nrm=None):
        return lib.lib.pn2_icp(n, lib.ptr(pts), None, n, lib.ptr(pts), None, nrm, r, est, init, it, tol, tol, lib.ptr(corr),
                               lib.ptr(res), lib.ptr(trace), lib.ptr(hdr), workspace, nbytes, lib.stream_ptr())
    bad = np.eye(4)
    bad[1, 2] = np.inf
    assert call(nbytes=need - 1) == -1 and call(nbytes=16) == -1 and call(workspace=ws.data_ptr() + off + 128) == -1
    assert call(it=-1) == -1 and call(r=float("nan")) == -1 and call(n=0) == -1 and call(est=2) == -1 and call(tol=-1.0) == -1
    assert call(init=_matrix(bad)) == -1 and call(corr=None) == -2 and call(est=1) == -2
    torch.cuda.synchronize()
    assert all((o[0] == POISON).all() for o in outs) and (ws == POISON).all()
    assert call() == 0  # the same buffers, accepted
    torch.cuda.synchronize()
    assert _payload(outs[0][0], 4 * n, "correspondence").view(np.int32).tolist() == [0] * n  # a hundred duplicates: index 0
    assert _payload(outs[3][0], 32, "header").view(np.int32).tolist() == [0, n, n, n, 1, 1, 0, 0]  # (M = 0: no rotation, the identity, and nothing changes)


# ---- the wrappers, the KITTI method, the example ---------------------------------------------------------------------------------
def test_wrappers_and_kitti_method(pn2, cuda, monkeypatch):
    import torch
    src, tgt, nrm = moved_corner()
    d_src, d_tgt = torch.from_numpy(src).to(cuda), torch.from_numpy(tgt).to(cuda)

    def same(reg, want, trace=False):
        assert isinstance(reg, pn2.RegistrationResult) and reg.correspondence.device == cuda and reg.correspondence.dtype == torch.int32
        assert reg.transformation.dtype == np.float64 and reg.transformation.tobytes() == want.result[:16].tobytes()
        assert (reg.fitness, reg.inlier_rmse) == (want.result[16], want.result[17])
        assert (reg.status, reg.iterations, reg.converged) == (want.header[0], want.header[4], bool(want.header[5]))
        assert reg.correspondence.cpu().numpy().tobytes() == want.correspondence.tobytes()
        if trace:
            assert reg.trace.tobytes() == want.trace[:want.header[4] + 1].tobytes()
        else:
            assert reg.trace is None

    p2p = R.icp(src, tgt, 0.5)
    same(pn2.registration_icp(d_src, d_tgt, 0.5), p2p)
    same(pn2.registration_icp(src.astype(np.float64), tgt, np.float64(0.5), trace=True), p2p, True)  # numpy, float64: cast
    p2l = R.icp(src, tgt, 0.5, 1, target_normals=nrm)
    same(pn2.registration_icp(d_src, d_tgt, 0.5, estimation="point_to_plane", target_normals=nrm, trace=True), p2l, True)
    init = rigid([0, 1, 0], 1.0, [0.05, 0, 0])
    same(pn2.registration_icp(d_src, d_tgt, 0.5, init=torch.from_numpy(init), max_iteration=2, relative_fitness=0, relative_rmse=0),
         R.icp(src, tgt, 0.5, 0, init, 2, 0.0, 0.0))
    ev = pn2.evaluate_registration(d_src, d_tgt, 0.5, init=init)
    same(ev, R.icp(src, tgt, 0.5, 0, init, 0))
    assert ev.iterations == 0 and np.array_equal(ev.transformation, init)
    rs = np.random.RandomState(9)
    slab, tlab = rs.randint(-1, 4, 400), rs.randint(-1, 4, 400)
    only = lambda lab: np.where(np.isin(lab, [1, 3]), lab, -1)  # noqa: E731
    same(pn2.registration_icp(d_src, d_tgt, 0.5, source_labels=slab, target_labels=torch.from_numpy(tlab).to(cuda), classes=[3, 1]),
         R.icp(src, tgt, 0.5, source_labels=only(slab), target_labels=only(tlab)))
    moved = pn2.transform_points(d_src, p2p.result[:16].reshape(4, 4))
    assert moved.device == cuda and moved.dtype == torch.float32
    assert moved.cpu().numpy().tobytes() == R.transform_points(src, p2p.result[:16].reshape(4, 4)).tobytes()
    assert np.abs(moved.cpu().numpy() - tgt).max() < 1e-5
    assert tuple(pn2.transform_points(d_src[:0], np.eye(4)).shape) == (0, 3)
    # nothing to register, and a target too wide for the grid
    none = pn2.registration_icp(d_src[:0], d_tgt, 0.5, init=init)
    assert none.correspondence.shape == (0,) and np.array_equal(none.transformation, init) and none.fitness == 0.0
    wide = torch.tensor([[0.0, 0, 0], [1e7, 0, 0]], device=cuda)
    assert pn2.registration_icp(d_src, wide, 1.0).status == 1
    # the KITTI method: frames are (cnt,3) float64 on the device
    prev = type("Frame", (), {"points": d_tgt.double()})()
    this = type("Frame", (), {"points": d_src.double()})()
    predictor = object.__new__(pn2.kitti_predict.PredictInterpolator)  # the method uses none of the network's state
    same(predictor.align_frames(prev, this, 0.5), p2p)
    same(predictor.align_frames(prev, this, 0.5, prev_dense_labels=tlab, dense_labels=slab, classes=[1, 3]),
         R.icp(src, tgt, 0.5, source_labels=only(slab), target_labels=only(tlab)))
    est = pn2.estimate_normals(d_tgt, 0.6, viewpoint=(0, 0, 0)).cpu().numpy()
    reg = predictor.align_frames(prev, this, 0.5, estimation="point_to_plane", normal_radius=0.6, trace=True)
    same(reg, R.icp(src, tgt, 0.5, 1, target_normals=est), True)
    assert reg.status == 0 and np.abs(reg.transformation - TRUTH).max() < 1e-3  # (estimated normals: a looser pose, still the motion)
    # a capturing stream is refused by the wrapper, before the library is touched (never by capturing)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capturing"):
        pn2.registration_icp(d_src, d_tgt, 0.5)
    with pytest.raises(RuntimeError, match="capturing"):
        predictor.align_frames(prev, this, 0.5)


def test_example(pn2, cuda, tmp_path):
    out = str(tmp_path / "frames")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "register_frames.py"), "--synthetic", "--points", "3000",
                          "--out", out, "--width", "320", "--height", "200"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    spec = importlib.util.spec_from_file_location("register_frames_example", os.path.join(ROOT, "examples", "register_frames.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    frames, poses = example.synthetic(3000)
    assert len(frames) == 3 and len(poses) == 3 and np.array_equal(poses[0], np.eye(4))
    lines = [line for line in run.stdout.splitlines() if line.startswith("frame ")]
    assert len(lines) == 4, run.stdout  # frames 1 and 2, both estimators
    for line in lines:
        angle, dist = float(line.split("error")[1].split()[0]), float(line.split("deg,")[1].split()[0])
        assert angle < 0.5 and dist < 0.05, line
    with open(os.path.join(out, "map.png"), "rb") as f:
        png = f.read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", png[16:24]) == (320, 200)
