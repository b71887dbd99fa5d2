"""pn2_linear_pool_packed (csrc/pn2_linear.hip): the pooled last layer of a [128, 128, wide] SA level on the LIVE ball-query rows
only.  Every output must have the BITS (compared as int32, so that a -0 would show) of pn2_linear(..., relu = 1, pool = 32) on the
same x, whatever the index table, and nothing may be stored outside the output.

The reference.  pn2_linear chooses its kernel by the row count: up to 2048 rows, and for a few hundred rows more, it splits the
contraction between waves and adds the partial sums afterwards, which rounds differently from its LDS-tiled kernel (one fmaf
chain over k) that takes every shape from 8192 rows on.  The packed kernel replaces the LDS-tiled kernel (the route starts far
above 4096 rows) and contracts in that kernel's order.  So the small group counts below are compared with pn2_linear on the same
rows REPEATED up to 8192 rows (whole groups; an output row depends on its own 32 input rows only): `_reference`.  From 8192 rows
on the reference is the plain call (test_plain_reference_from_8192_rows_on, the module test).

x is built by gathering random source rows through idx, so the rows behind a padded index entry are copies of the group's first
row: the entry point's precondition.  The kernel takes blocks of 8 consecutive groups at these sizes (BLOCK); the tables aim at
the classifier and at the tile list of one block, and each test asserts on its INPUT that the table packs as intended; the
larger blocks (16 at the benchmark's SA3, up to the cap of 64) have a test of their own, test_large_blocks_same_bits."""
import numpy as np
import pytest
import torch

import test_sa_row_packing_gpu as r07
from conftest import s_scene
from test_layers_gpu import close, layer_dicts, randomize_bn
from test_sa_row_packing_gpu import packing  # noqa: F401  (fixture: packing(on, where), back to the default afterwards)
from test_sa_wide_row_packing_cpu import _tool

pytestmark = pytest.mark.gpu

T = r07.T
TOOL = _tool()
BLOCK = 8        # groups per workgroup of the packed kernel below 2048 groups (pn2_linear_pool_packed's `blk`)
REF_ROWS = 8192  # from here on pn2_linear(pool = 32) runs its LDS-tiled kernel for cout = 128 and 256
CIN = 128
GUARD = 4        # NaN rows in front of and behind the output
NSRC = 64        # source rows per cloud


def _scattered(rs, n):
    """[5, 7, 5, 5, 9, 5, ...]: equal entries that are not contiguous -- live = 5 (the last differing position + 1), although
    only three values occur"""
    r = np.full(32, 5, dtype=np.int32)
    r[1], r[4] = 7, 9
    return r


def _of_class(rs, n, cls):
    lo, hi = {8: (1, 8), 16: (9, 16), 32: (17, 32)}[cls]
    return r07._row(rs, n, lo + rs.randint(0, hi - lo + 1))


def _edges_table(groups, n, seed):
    """live counts 1, 8, 9, 16, 17, 31, 32 and the scattered row, in turn"""
    rs = np.random.RandomState(seed)
    makers = [lambda: r07._row(rs, n, 1), lambda: r07._row(rs, n, 8), lambda: r07._row(rs, n, 9), lambda: r07._row(rs, n, 16),
              lambda: r07._row(rs, n, 17), lambda: r07._row(rs, n, 31), lambda: r07._row(rs, n, 32), lambda: _scattered(rs, n)]
    return np.stack([makers[(g + seed) % len(makers)]() for g in range(groups)])


def _blocks_table(blocks, n, seed):
    """blocks = [(n8, n16, n32), ...]: the groups of each kernel block, shuffled inside it; every block but the last is filled up
    to BLOCK groups with class 32"""
    rs = np.random.RandomState(seed)
    rows = []
    for i, (n8, n16, n32) in enumerate(blocks):
        if i + 1 < len(blocks):
            n32 = BLOCK - n8 - n16
        assert 0 < n8 + n16 + n32 <= BLOCK and n32 >= 0
        blk = [_of_class(rs, n, 8) for _ in range(n8)] + [_of_class(rs, n, 16) for _ in range(n16)] + [_of_class(rs, n, 32) for _ in range(n32)]
        rows += [blk[j] for j in rs.permutation(len(blk))]
    return np.stack(rows)


def _tiles(idx_np, block=BLOCK):
    return TOOL.packed_tiles(TOOL.classes(idx_np.reshape(-1, 32)), block)


def _case(rs, idx_np, cout, dev, bias_shift=0.0):
    """idx (b, m, 32) -> x (b * m * 32, CIN) gathered from each cloud's own source rows, w, bias"""
    b = idx_np.shape[0]
    src = rs.randn(b, NSRC, CIN).astype(np.float32)
    x = src[np.arange(b)[:, None, None], idx_np].reshape(-1, CIN)
    w = (rs.randn(CIN, cout) / np.sqrt(CIN)).astype(np.float32)
    bias = (0.1 * rs.randn(cout) + bias_shift).astype(np.float32)
    return T(x, dev), T(idx_np, dev), T(w, dev), T(bias, dev)


def _reference(pn2, x, w, bias):
    """pn2_linear(..., relu = 1, pool = 32) on the same rows, repeated up to REF_ROWS rows where there are fewer (module docstring)"""
    rows = x.shape[0]
    if rows < REF_ROWS:
        x = x.repeat(-(-REF_ROWS // rows), 1)[:REF_ROWS].contiguous()
    return pn2.util.tf_util.hip_linear(x, w, bias, relu=True, pool=32)[:rows // 32]


def _packed(pn2, x, idx, w, bias, nsample=32, relu=1, cout=None):
    """the entry point itself, into a slice of a NaN-filled buffer -> (taken, y, guard rows)"""
    L = pn2._lib
    groups = idx.shape[0] * idx.shape[1]
    cout = w.shape[1] if cout is None else cout
    buf = torch.full((groups + 2 * GUARD, cout), float("nan"), dtype=torch.float32, device=x.device)
    y = buf[GUARD:GUARD + groups]
    ok = L.launch("pn2_linear_pool_packed", x, groups, nsample, x.shape[1], cout, L.ptr(x), L.ptr(idx), L.ptr(w), L.ptr(bias),
                  relu, L.ptr(y), may_refuse=True)
    torch.cuda.synchronize()
    return ok, y, torch.cat([buf[:GUARD], buf[GUARD + groups:]])


def _same_bits(got, ref):
    assert not torch.isnan(got).any(), "the packed kernel left rows unwritten"
    a, b = got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)
    assert torch.equal(a, b), "packed != pn2_linear: %d of %d values differ, max |diff| %.3e" % (
        int((a != b).sum()), a.numel(), float((got - ref).abs().max()))


def _check(pn2, packing, idx_np, cout, seed, bias_shift=0.0):  # noqa: F811
    dev = torch.device("cuda:0")
    packing(True, dev)
    x, idx, w, bias = _case(np.random.RandomState(seed), idx_np, cout, dev, bias_shift)
    ok, y, guard = _packed(pn2, x, idx, w, bias)
    assert ok, "refused"
    assert torch.isnan(guard).all(), "a store outside the output"
    _same_bits(y, _reference(pn2, x, w, bias))
    return y


# 130 groups = 2 clouds x 65: 17 blocks, the last one short, and tiles that mix the clouds
SHAPES = [(1, 1), (1, 3), (1, 63), (1, 64), (1, 65), (2, 65)]


@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("b,m", SHAPES)
def test_live_count_edges_same_bits(pn2, cuda, packing, b, m, cout):  # noqa: F811
    """live = 1, 8, 9, 16, 17, 31, 32 and a group whose equal entries are not contiguous, at every group count"""
    idx_np = _edges_table(b * m, NSRC, seed=m + cout).reshape(b, m, 32)
    live = r07.live_slots(idx_np).reshape(-1)
    if b * m >= 8:
        assert set(live.tolist()) == {1, 5, 8, 9, 16, 17, 31, 32}
        assert _tiles(idx_np) < b * m
    _check(pn2, packing, idx_np, cout, seed=b * 1009 + m)


def test_scattered_row_is_classified_by_its_last_differing_position():
    r = _scattered(None, NSRC)
    assert list(r[:6]) == [5, 7, 5, 5, 9, 5] and len(set(r.tolist())) == 3 and int(r07.live_slots(r)) == 5


# (name, blocks of (class 8, class 16, class 32) groups, tiles the packer must form)
BLOCKS = [("one_8", [(1, 0, 0)], 1), ("four_8", [(4, 0, 0)], 1), ("five_8", [(5, 0, 0)], 2),
          ("one_16", [(0, 1, 0)], 1), ("three_16", [(0, 3, 0)], 2),
          ("promote", [(5, 1, 0)], 2),            # the class-16 group takes the fifth class-8 group along: 1 + 1 tiles, not 1 + 2
          ("promote_3_16", [(1, 3, 2)], 2 + 2),   # 16 16 | 16 8 | 32 | 32
          ("no_promote", [(2, 1, 0)], 2),         # n8 % 4 == 2: nothing to save
          ("all_32", [(0, 0, 8), (0, 0, 3)], 11),
          ("full_then_short", [(4, 2, 2), (8, 0, 0), (0, 8, 0), (3, 1, 0)], 4 + 2 + 4 + 2),
          ("short_tail_of_one", [(2, 3, 3), (1, 0, 0)], 1 + 2 + 3 + 1)]


@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("name,blocks,tiles", BLOCKS, ids=[b_[0] for b_ in BLOCKS])
def test_block_compositions_same_bits(pn2, cuda, packing, name, blocks, tiles, cout):  # noqa: F811
    idx_np = _blocks_table(blocks, NSRC, seed=len(name))
    assert _tiles(idx_np) == tiles
    _check(pn2, packing, idx_np.reshape(1, -1, 32), cout, seed=len(name) + cout)


def test_maxima_below_zero_give_plus_zero(pn2, cuda, packing):  # noqa: F811
    """a bias far below the products: most maxima are negative in front of the ReLU, the output is +0 there (bit pattern 0)"""
    idx_np = _edges_table(65, NSRC, seed=2).reshape(1, 65, 32)
    y = _check(pn2, packing, idx_np, 256, seed=77, bias_shift=-2.0)
    zeros = y == 0
    assert 0.25 < float(zeros.float().mean()) < 1.0, float(zeros.float().mean())
    assert int(y.contiguous().view(torch.int32)[zeros].abs().max()) == 0, "a -0 in the output"


def test_plain_reference_from_8192_rows_on(pn2, cuda, packing):  # noqa: F811
    """257 groups = 8224 rows: pn2_linear's own launch on exactly these rows is the reference (nothing repeated), 33 blocks with a
    last block of one group"""
    dev = torch.device("cuda:0")
    packing(True, dev)
    idx_np = np.concatenate([r07._table("mixed", 200, NSRC, seed=4), _edges_table(57, NSRC, seed=5)]).reshape(1, 257, 32)
    assert _tiles(idx_np) < 0.8 * 257
    for cout in (128, 256):
        x, idx, w, bias = _case(np.random.RandomState(cout), idx_np, cout, dev)
        assert x.shape[0] >= REF_ROWS
        ok, y, guard = _packed(pn2, x, idx, w, bias)
        assert ok and torch.isnan(guard).all()
        _same_bits(y, pn2.util.tf_util.hip_linear(x, w, bias, relu=True, pool=32))


# (b, m, cout) -> the launcher's block = clamp(ceil(b * m * (cout / 64) / 256), 8, 64)
BIG = [(16, 64, 256, 16),    # SA3 of the benchmark: 1024 groups, blocks of 16 (two classifier passes per wave pair)
       (2, 700, 128, 11),    # a block size that is no multiple of 4 or 8, last block short (1400 = 127 * 11 + 3)
       (4, 1024, 256, 64),   # 4096 groups: exactly the cap, tile lists of up to 64 tiles
       (1, 5001, 256, 64)]   # the cap clamps (79 asked for), last block of 9 groups


@pytest.mark.parametrize("b,m,cout,block", BIG)
def test_large_blocks_same_bits(pn2, cuda, packing, b, m, cout, block):  # noqa: F811
    """block sizes above 8 up to the cap of 64; the reference is pn2_linear on exactly these rows (all >= 8192)"""
    groups = b * m
    assert block == min(64, max(8, -(-groups * (cout // 64) // 256)))
    packing(True, cuda)
    idx_np = np.concatenate([r07._table("mixed", groups - 100, NSRC, seed=m), _edges_table(100, NSRC, seed=b)]).reshape(b, m, 32)
    assert _tiles(idx_np, block) < 0.8 * groups
    x, idx, w, bias = _case(np.random.RandomState(m + cout), idx_np, cout, cuda)
    assert x.shape[0] >= REF_ROWS
    ok, y, guard = _packed(pn2, x, idx, w, bias)
    assert ok and torch.isnan(guard).all()
    _same_bits(y, pn2.util.tf_util.hip_linear(x, w, bias, relu=True, pool=32))


def test_switch_off_refuses_and_the_wrapper_launches_pn2_linear(pn2, cuda, packing):  # noqa: F811
    """257 groups (8224 rows): pn2_linear runs its LDS-tiled kernel here, so switch on and switch off must agree in every bit"""
    tfu = pn2.util.tf_util
    G = 257
    idx_np = _edges_table(G, NSRC, seed=9).reshape(1, G, 32)
    x, idx, w, bias = _case(np.random.RandomState(3), idx_np, 256, cuda)
    packing(True, cuda)
    ok, on, _ = _packed(pn2, x, idx, w, bias)
    assert ok
    packing(False, cuda)
    ok, off, guard = _packed(pn2, x, idx, w, bias)
    assert not ok and torch.isnan(off).all() and torch.isnan(guard).all(), "switched off, the entry point must launch nothing"
    store = tfu.set_default_store(tfu.VariableStore(device=cuda, seed=11))
    assert store is not None
    outs = {}
    for sw in (True, False):
        packing(sw, cuda)
        pn2._lib.lib.trace = calls = []
        try:
            with torch.no_grad():
                outs[sw] = tfu.conv2d(x.reshape(1, G, 32, CIN), 256, [1, 1], padding="VALID", stride=[1, 1], bn=True,
                                      is_training=False, scope="sw/conv2", pool=32, pool_idx=idx)
        finally:
            pn2._lib.lib.trace = None
        names = [c_[0] for c_ in calls]
        assert ("pn2_linear" in names) == (not sw), names
        assert "pn2_linear_pool_packed" in names  # asked first either way; refused (nothing launched) with the switch off
    assert outs[True].shape == (1, G, 1, 256)
    _same_bits(outs[True].reshape(G, 256), outs[False].reshape(G, 256))


@pytest.mark.parametrize("what", ["nsample_16", "cout_96", "misaligned_x", "relu_0", "no_bias"])
def test_refusals_launch_nothing(pn2, cuda, packing, what):  # noqa: F811
    packing(True, cuda)
    idx_np = _edges_table(16, NSRC, seed=1).reshape(1, 16, 32)
    x, idx, w, bias = _case(np.random.RandomState(1), idx_np, 128, cuda)
    kw = {}
    if what == "nsample_16":
        kw["nsample"] = 16
    elif what == "cout_96":
        kw["cout"] = 96
    elif what == "misaligned_x":
        shifted = torch.empty(x.numel() + 1, dtype=torch.float32, device=cuda)
        shifted[1:] = x.reshape(-1)
        x = shifted[1:].reshape(x.shape)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    elif what == "relu_0":
        kw["relu"] = 0
    else:
        bias = None
    ok, y, guard = _packed(pn2, x, idx, w, bias, **kw)
    assert not ok, "PN2_EUNSUP expected"
    assert torch.isnan(y).all() and torch.isnan(guard).all(), "a refused call must launch nothing"


def test_sa_module_at_the_route_threshold(pn2, oracle, cuda, packing):  # noqa: F811
    """pointnet_sa_module([128, 128, 256]) at the smallest row count the route takes: the packed launch is in the trace, the
    output has the bits of the un-packed route (pn2_linear's LDS-tiled kernel at this size) and is within 1e-5 of the oracle"""
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    b, n, c = 2, 1024, 128
    m = pu.POOL_PACKED_MIN_ROWS // (b * 32)
    assert b * m * 32 == pu.POOL_PACKED_MIN_ROWS and m <= n
    rs = np.random.RandomState(m)
    xyz = s_scene(m, b, n)
    pts = rs.randn(b, n, c).astype(np.float32)
    store = tfu.set_default_store(tfu.VariableStore(device=cuda, seed=61))
    kw = dict(npoint=m, radius=0.5, nsample=32, mlp=[128, 128, 256], mlp2=None, group_all=False, is_training=False,
              bn_decay=None, scope="sa")
    pu.pointnet_sa_module(T(xyz, cuda), T(pts, cuda), **kw)
    randomize_bn(store, 62)
    outs = {}
    for on in (True, False):
        packing(on, cuda)
        pn2._lib.lib.trace = calls = []
        try:
            _, outs[on], idx = pu.pointnet_sa_module(T(xyz, cuda), T(pts, cuda), **kw)
        finally:
            pn2._lib.lib.trace = None
        names = [c_[0] for c_ in calls]
        assert ("pn2_linear_pool_packed" in names) == on, names
        pooled = [c_ for c_ in calls if c_[0] == "pn2_linear" and c_[1][0] == b * m * 32]  # (the hoisted product is a pn2_linear too)
        assert len(pooled) == (0 if on else 1), calls
    idx_np = idx.cpu().numpy()
    print("class shares (8, 16, 32) %.2f %.2f %.2f" % r07.class_shares(idx_np))
    assert r07.class_shares(idx_np)[2] < 0.9, "the geometry must leave rows to pack"
    _same_bits(outs[True].reshape(b * m, 256), outs[False].reshape(b * m, 256))
    _, ref, ridx = oracle.sa_module(xyz, pts, m, 0.5, 32, layer_dicts(store, "sa", ["conv0", "conv1", "conv2"]))
    assert np.array_equal(idx_np, ridx)
    close(outs[True].cpu().numpy(), ref)
