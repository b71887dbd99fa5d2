"""Row packing of the pooled K = 32 set-abstraction kernels (csrc/pn2_sa_fused.hip, PACK): packing on vs. off through the
switch must give the SAME BITS -- no value is computed differently, a padded row is a copy of row 0 of its group and the max
does not count copies.  Real geometry at the full size of configs[1] (where most rows are padding: asserted on the inputs, so
that no case passes because nothing packed) and hand-made index tables that aim at the classifier and the packer."""
import numpy as np
import pytest
import torch

from benchlib import inputs as bench_inputs

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def live_slots(idx):
    """(..., 32) index rows -> 1 + the last position that differs from position 0"""
    diff = idx != idx[..., :1]
    last = 31 - np.argmax(diff[..., ::-1], axis=-1)
    return np.where(diff.any(axis=-1), last + 1, 1)


def class_shares(idx):
    live = live_slots(idx).reshape(-1)
    return np.mean(live <= 8), np.mean((live > 8) & (live <= 16)), np.mean(live > 16)


@pytest.fixture
def packing(pn2):
    """packing(on, where): set the module flag and tell the library; back to the default afterwards"""
    pu = pn2.util.pointnet_util

    def set_(on, where):
        pu.USE_SA_ROW_PACKING = bool(on)
        pu._sync_sa_row_packing(where)

    yield set_
    pu.USE_SA_ROW_PACKING = True
    if torch.cuda.is_available():
        pu._sync_sa_row_packing(torch.device("cuda:0"))


def _weights(rs, cin, mlp, dev):
    ws, bs = [], []
    for cout in mlp:
        ws.append(T((rs.randn(cin, cout) / np.sqrt(cin)).astype(np.float32), dev))
        bs.append(T((0.1 * rs.randn(cout)).astype(np.float32), dev))
        cin = cout
    return ws, bs


def _run_max_fused(pn2, xyz, new_xyz, pts, idx, mlp, ws, bs):
    L = pn2._lib
    b, n, _ = xyz.shape
    m = idx.shape[1]
    c = 0 if pts is None else pts.shape[2]
    out = torch.full((b, m, mlp[-1]), float("nan"), dtype=torch.float32, device=xyz.device)
    L.launch("pn2_sa_mlp_max_fused", xyz, b, n, m, 32, c, L.ptr(xyz), L.ptr(new_xyz), L.ptr(pts), L.ptr(idx), len(mlp),
             L.int_array(mlp), L.ptr_table(ws), L.ptr_table(bs), L.ptr(out))
    return out


def _run_fused_pre(pn2, xyz, new_xyz, zf, idx, mlp, ws, bs):
    L = pn2._lib
    b, n, _ = xyz.shape
    m = idx.shape[1]
    out = torch.full((b, m, mlp[-1]), float("nan"), dtype=torch.float32, device=xyz.device)
    L.launch("pn2_sa_mlp_fused_pre", xyz, b, n, m, 32, L.ptr(xyz), L.ptr(new_xyz), L.ptr(zf), L.ptr(idx), len(mlp),
             L.int_array(mlp), L.ptr_table(ws), L.ptr_table(bs), 1, L.ptr(out))
    return out


def _on_off(packing, run):
    packing(False, torch.device("cuda:0"))
    off = run()
    packing(True, torch.device("cuda:0"))
    on = run()
    torch.cuda.synchronize()
    assert not torch.isnan(off).any(), "the un-packed kernel left rows unwritten"
    assert not torch.isnan(on).any(), "the packed kernel left rows unwritten"
    assert torch.equal(on, off), "packed != un-packed: %d of %d values differ" % (int((on != off).sum()), on.numel())


# ---- real geometry, full size ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gen", ["s_scene", "s_randn", "s_dup25"])
def test_sa1_sa2_full_size_same_bits(pn2, cuda, packing, gen):
    """SA1 ([32,32,64] on xyz + rgb, both entry points) and SA2 ([64,64,128], hoisted and not) of configs[1], B = 16 x 8192,
    with the library's own sampling and ball query."""
    pu = pn2.util.pointnet_util
    hp = pn2.model.SEMANTIC_HYPERPARAMS
    pc = T(getattr(bench_inputs, gen)(0, 16, 8192), cuda)
    xyz, rgb = pc[:, :, 0:3].contiguous(), pc[:, :, 3:6].contiguous()
    rs = np.random.RandomState(5)
    with torch.no_grad():
        l1_xyz, idx1 = pu.sa_geometry(xyz, hp["l1_npoint"], hp["l1_radius"], hp["l1_nsample"])
        l2_xyz, idx2 = pu.sa_geometry(l1_xyz, hp["l2_npoint"], hp["l2_radius"], hp["l2_nsample"])
    s1, s2 = class_shares(idx1.cpu().numpy()), class_shares(idx2.cpu().numpy())
    print("%s: class shares (8, 16, 32)  SA1 %.2f %.2f %.2f   SA2 %.2f %.2f %.2f" % ((gen,) + s1 + s2))
    if gen in ("s_scene", "s_dup25"):  # a condition on the inputs: the comparison below is about tiles that did pack
        assert s1[0] + s1[1] >= 0.5 and s2[0] + s2[1] >= 0.5, (s1, s2)
    mlp1, mlp2 = [32, 32, 64], [64, 64, 128]
    w1, b1 = _weights(rs, 6, mlp1, cuda)
    _on_off(packing, lambda: _run_max_fused(pn2, xyz, l1_xyz, rgb, idx1, mlp1, w1, b1))
    # the in-place form the model uses (xyz / rgb read where they lie in the (b, n, 6) batch), through the module flag
    store = pn2.util.tf_util.set_default_store(pn2.util.tf_util.VariableStore(device=cuda, seed=3))
    assert store is not None
    with torch.no_grad():
        _on_off(packing, lambda: pu._sa_fused_inference(pc[:, :, 0:3], l1_xyz, pc[:, :, 3:6], idx1, mlp1, True, "pk_sa1/conv%d"))
    feat = T(rs.randn(16, hp["l1_npoint"], 64).astype(np.float32), cuda)
    w2, b2 = _weights(rs, 3 + 64, mlp2, cuda)
    _on_off(packing, lambda: _run_max_fused(pn2, l1_xyz, l2_xyz, feat, idx2, mlp2, w2, b2))
    zf = T(rs.randn(16 * hp["l1_npoint"], 64).astype(np.float32), cuda)
    w2x = [w2[0][:3].contiguous()] + w2[1:]
    _on_off(packing, lambda: _run_fused_pre(pn2, l1_xyz, l2_xyz, zf, idx2, mlp2, w2x, b2))


# ---- hand-made index tables -----------------------------------------------------------------------------------------------

def _row(rs, n, live):
    """a 32-entry row with exactly `live` live slots: position live - 1 differs from position 0, everything behind is padding"""
    first = rs.randint(0, n)
    r = np.full(32, first, dtype=np.int32)
    if live > 1:
        r[1:live - 1] = rs.randint(0, n, live - 2)
        r[live - 1] = (first + 1 + rs.randint(0, n - 1)) % n
    return r


def _late_odd(rs, n):
    """idx[0] everywhere except position 20: class 32, although only two values occur"""
    r = _row(rs, n, 1)
    r[20] = (r[0] + 1) % n
    return r


def _table(kind, groups, n, seed):
    rs = np.random.RandomState(seed)
    if kind == "random":  # nothing packs
        return rs.randint(0, n, (groups, 32)).astype(np.int32)
    if kind == "zeros":  # what the ball query writes for an empty ball
        return np.zeros((groups, 32), dtype=np.int32)
    if kind == "all8":
        return np.stack([_row(rs, n, 1 + rs.randint(0, 8)) for _ in range(groups)])
    if kind == "lone16":  # one class-16 group among class-32 ones
        t = rs.randint(0, n, (groups, 32)).astype(np.int32)
        t[:, 31] = (t[:, 0] + 1) % n
        for g in (5, groups // 2 + 1, groups - 1):
            t[g] = _row(rs, n, 16)
        return t
    assert kind == "mixed"
    makers = [lambda: _row(rs, n, 1), lambda: _row(rs, n, 8), lambda: _row(rs, n, 9), lambda: _row(rs, n, 16),
              lambda: _row(rs, n, 17), lambda: _row(rs, n, 32), lambda: _late_odd(rs, n),
              lambda: np.zeros(32, dtype=np.int32), lambda: rs.randint(0, n, 32).astype(np.int32),
              lambda: _row(rs, n, 2 + rs.randint(0, 6)), lambda: _row(rs, n, 10 + rs.randint(0, 6))]
    return np.stack([makers[rs.randint(0, len(makers))]() for _ in range(groups)])


def test_row_maker_hits_the_class_edges():
    rs = np.random.RandomState(0)
    for live in (1, 8, 9, 16, 17, 32):
        assert live_slots(_row(rs, 100, live)) == live
    assert live_slots(_late_odd(rs, 100)) == 21
    assert live_slots(np.zeros(32, dtype=np.int32)) == 1


# (b, m): what the launch makes of them -- centres per block, blocks per workgroup -- is in launch_chain / pack_block
SHAPES = [(16, 1024),   # the SA1 count: 32 centres per block, one block per workgroup, XCD ranges
          (1, 16424),   # 33 centres per block (not a multiple of 4), the last block of every XCD range holds 7
          (1, 16391),   # a centre count that is no multiple of 8: no XCD ranges, the last block is ragged
          (2, 20000),   # 64 centres per block (the cap) and workgroups that take two blocks
          (2, 64),      # a small call: 4 centres per block
          (1, 7)]       # fewer centres than one workgroup has waves


@pytest.mark.parametrize("kind", ["mixed", "all8", "lone16", "random", "zeros"])
@pytest.mark.parametrize("b,m", SHAPES)
def test_hand_made_tables_same_bits(pn2, cuda, packing, kind, b, m):
    n = 512
    rs = np.random.RandomState(b * 100003 + m)
    idx_np = _table(kind, b * m, n, seed=m + len(kind)).reshape(b, m, 32)
    if kind == "all8":
        assert class_shares(idx_np)[0] == 1.0
    if kind == "random":
        assert class_shares(idx_np)[2] > 0.95
    xyz = T(rs.uniform(-1, 1, (b, n, 3)).astype(np.float32), cuda)
    new_xyz = T(rs.uniform(-1, 1, (b, m, 3)).astype(np.float32), cuda)
    idx = T(idx_np, cuda)
    # SA1's kernel: [32,32,64] on 3 feature channels (the un-vectorised gather)
    pts3 = T(rs.randn(b, n, 3).astype(np.float32), cuda)
    w, bias = _weights(rs, 6, [32, 32, 64], cuda)
    _on_off(packing, lambda: _run_max_fused(pn2, xyz, new_xyz, pts3, idx, [32, 32, 64], w, bias))
    # the 16-byte feature gather, one layer
    pts8 = T(rs.randn(b, n, 8).astype(np.float32), cuda)
    w, bias = _weights(rs, 11, [64], cuda)
    _on_off(packing, lambda: _run_max_fused(pn2, xyz, new_xyz, pts8, idx, [64], w, bias))
    # SA2's kernel: [64,64,128] with the feature part of layer 1 hoisted
    zf = T(rs.randn(b * n, 64).astype(np.float32), cuda)
    w, bias = _weights(rs, 3, [64, 64, 128], cuda)
    _on_off(packing, lambda: _run_fused_pre(pn2, xyz, new_xyz, zf, idx, [64, 64, 128], w, bias))


def test_packed_output_matches_float64(pn2, cuda, packing):
    """the packed kernel against a float64 evaluation of the same chain (the on / off comparison alone would not see an error
    that both share)"""
    b, n, m = 2, 512, 300
    rs = np.random.RandomState(11)
    idx_np = _table("mixed", b * m, n, seed=1).reshape(b, m, 32)
    xyz_np = rs.uniform(-1, 1, (b, n, 3)).astype(np.float32)
    new_np = rs.uniform(-1, 1, (b, m, 3)).astype(np.float32)
    pts_np = rs.randn(b, n, 3).astype(np.float32)
    mlp = [32, 32, 64]
    w, bias = _weights(rs, 6, mlp, cuda)
    packing(True, cuda)
    got = _run_max_fused(pn2, T(xyz_np, cuda), T(new_np, cuda), T(pts_np, cuda), T(idx_np, cuda), mlp, w, bias).cpu().numpy()
    bi = np.arange(b)[:, None, None]
    x = np.concatenate([xyz_np[bi, idx_np] - new_np[:, :, None, :], pts_np[bi, idx_np]], axis=-1).astype(np.float64)
    for wi, bv in zip(w, bias):
        x = np.maximum(x @ wi.cpu().numpy().astype(np.float64) + bv.cpu().numpy().astype(np.float64), 0.0)
    ref = x.max(axis=2)
    # fp32 dot products of at most 32 terms of order one: 1e-5 is the bound the layer tests hold the kernels to
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
