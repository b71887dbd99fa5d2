"""Row packing of the wide SA kernel (csrc/pn2_mlp_wide.hip, PACK; pn2_sa_mlp_wide and pn2_sa_mlp_wide_pre with pooling): packing
on vs. off through the process-wide switch must give the SAME BITS for any index table, store nothing outside the output, and both
must match float64.  The packer works on chunks of 256 consecutive groups, one workgroup per tile: the shapes aim at its edges
(one full chunk, fewer groups than waves, a ragged second chunk whose tiles mix clouds, two full chunks, a chunk of one group),
the tables at the classifier and the tile list (the r07 tables + the take-along rule + a short last tile).  Every comparison
asserts on its INPUT that the table packs (or, for `random`, that it does not): no case passes because nothing packed."""
import numpy as np
import pytest
import torch

import test_sa_row_packing_gpu as r07
from test_layers_gpu import close
from test_sa_wide_row_packing_cpu import _tool
from test_sa_row_packing_gpu import packing  # noqa: F401  (fixture: packing(on, where), back to the default afterwards)

pytestmark = pytest.mark.gpu

T = r07.T
CHUNK = 256


TOOL = _tool()


def wide_tiles(idx_np):
    """32-row tiles the packed wide kernel runs for this table (its chunk packer restated in tools/sa_row_packing_stats.py)"""
    cls = TOOL.classes(idx_np.reshape(-1, 32))
    return sum(len(TOOL.chunk_tiles(cls[lo:lo + CHUNK], lo)) for lo in range(0, len(cls), CHUNK))


def _chunk_counts(kind, cnt):
    """(class-8, class-16, class-32) groups of a chunk of cnt groups"""
    if kind == "take_along":  # exactly one class-16 group and 4k + 1 class-8 groups: the last class-8 group rides with the 16
        n8 = ((cnt - 2) // 4) * 4 + 1 if cnt >= 2 else 0
        return n8, 1, cnt - 1 - n8
    assert kind == "short8"   # a class-8 count that is no multiple of 4: the last class-8 tile has empty slots
    n8 = cnt - cnt // 4
    while n8 % 4 == 0:
        n8 -= 1
    return n8, 0, cnt - n8


def _table(kind, groups, n, seed):
    if kind not in ("take_along", "short8"):
        return r07._table(kind, groups, n, seed)
    rs = np.random.RandomState(seed)
    rows = []
    for lo in range(0, groups, CHUNK):
        n8, n16, n32 = _chunk_counts(kind, min(CHUNK, groups - lo))
        chunk = ([r07._row(rs, n, 1 + rs.randint(0, 8)) for _ in range(n8)] + [r07._row(rs, n, 9 + rs.randint(0, 8)) for _ in range(n16)]
                 + [r07._row(rs, n, 17 + rs.randint(0, 16)) for _ in range(n32)])
        rows += [chunk[i] for i in rs.permutation(len(chunk))]
    return np.stack(rows)


def test_chunk_tables_hit_the_packer_edges():
    for groups in (256, 7, 300, 512, 257):
        for kind in ("take_along", "short8"):
            cls = TOOL.classes(_table(kind, groups, 64, 3))
            for lo in range(0, groups, CHUNK):
                c = cls[lo:lo + CHUNK]
                n8, n16 = int((c == 8).sum()), int((c == 16).sum())
                assert (n8, n16, int((c == 32).sum())) == _chunk_counts(kind, len(c))
                if kind == "take_along":
                    assert n16 == 1 and (len(c) < 2 or n8 % 4 == 1)
                else:
                    assert n16 == 0 and n8 % 4 != 0


def _weights(rs, cin, widths, dev, zero_from=None):
    """dense layers; the first has cin rows (a multiple of 8), rows >= zero_from zero (the kernel's padding rows)"""
    ws, bs = [], []
    for i, cout in enumerate(widths):
        w = (rs.randn(cin, cout) / np.sqrt(cin)).astype(np.float32)
        if i == 0 and zero_from is not None:
            w[zero_from:] = 0.0
        ws.append(T(w, dev))
        bs.append(T((0.1 * rs.randn(cout)).astype(np.float32), dev))
        cin = cout
    return ws, bs


GUARD = 4  # NaN rows in front of and behind the output


def _launch(pn2, name, xyz, new_xyz, src, idx, widths, ws, bs):
    """pn2_sa_mlp_wide (src = points (b, n, c)) or pn2_sa_mlp_wide_pre (src = zf (b*n, widths[0])), pooled, into a slice of a
    larger NaN-filled buffer -> (output, guard rows)"""
    L = pn2._lib
    b, n, _ = xyz.shape
    m = idx.shape[1]
    wl = widths[-1]
    buf = torch.full((b * m + 2 * GUARD, wl), float("nan"), dtype=torch.float32, device=xyz.device)
    y = buf[GUARD:GUARD + b * m]
    args = (b, n, m, 32) + ((src.shape[2],) if name == "pn2_sa_mlp_wide" else ())
    L.launch(name, xyz, *args, L.ptr(xyz), L.ptr(new_xyz), L.ptr(src), L.ptr(idx), len(widths), L.int_array(widths), L.ptr_table(ws),
             L.ptr_table(bs), 1, L.ptr(y))
    return y.reshape(b, m, wl), torch.cat([buf[:GUARD], buf[GUARD + b * m:]])


def _on_off(packing, run):  # noqa: F811
    dev = torch.device("cuda:0")
    packing(False, dev)
    off, guard_off = run()
    packing(True, dev)
    on, guard_on = run()
    torch.cuda.synchronize()
    assert not torch.isnan(off).any(), "the un-packed kernel left rows unwritten"
    assert not torch.isnan(on).any(), "the packed kernel left rows unwritten"
    assert torch.isnan(guard_off).all() and torch.isnan(guard_on).all(), "a store outside the output"
    assert torch.equal(on, off), "packed != un-packed: %d of %d values differ" % (int((on != off).sum()), on.numel())


SHAPES = [(16, 16),   # one full chunk, SA4's own count
          (1, 7),     # fewer groups than waves
          (3, 100),   # two chunks, the second ragged (44 groups); tiles that mix clouds
          (2, 256),   # two full chunks
          (1, 257)]   # a chunk of one group
WIDTHS = [(256, 256, 512), (128, 128, 256), (128,)]  # (128,): the pooled epilogue follows the z-gather directly


@pytest.mark.parametrize("kind", ["mixed", "all8", "lone16", "random", "zeros", "take_along", "short8"])
@pytest.mark.parametrize("b,m", SHAPES)
def test_tables_same_bits_and_no_stray_stores(pn2, cuda, packing, kind, b, m):  # noqa: F811
    n, c = 64, 12
    groups = b * m
    rs = np.random.RandomState(b * 1009 + m)
    idx_np = _table(kind, groups, n, seed=m + len(kind)).reshape(b, m, 32)
    tiles = wide_tiles(idx_np)
    print("%s (%d, %d): %d tiles for %d groups" % (kind, b, m, tiles, groups))
    if kind == "random":
        assert tiles == groups
    elif kind == "all8":
        assert r07.class_shares(idx_np)[0] == 1.0 and tiles == sum((min(CHUNK, groups - lo) + 3) // 4 for lo in range(0, groups, CHUNK))
    elif kind in ("mixed", "zeros", "take_along", "short8"):
        assert tiles < groups
    xyz = T(rs.uniform(-1, 1, (b, n, 3)).astype(np.float32), cuda)
    new_xyz = T(rs.uniform(-1, 1, (b, m, 3)).astype(np.float32), cuda)
    idx = T(idx_np, cuda)
    assert idx.data_ptr() % 16 == 0
    pts = T(rs.randn(b, n, c).astype(np.float32), cuda)  # every cloud its own features: a wrong cloud base shows
    for widths in WIDTHS:
        ws, bs = _weights(rs, 16, widths, cuda, zero_from=c + 3)
        _on_off(packing, lambda: _launch(pn2, "pn2_sa_mlp_wide", xyz, new_xyz, pts, idx, widths, ws, bs))
        zf = T(rs.randn(b * n, widths[0]).astype(np.float32), cuda)
        ws, bs = _weights(rs, 8, widths, cuda, zero_from=3)
        _on_off(packing, lambda: _launch(pn2, "pn2_sa_mlp_wide_pre", xyz, new_xyz, zf, idx, widths, ws, bs))


def _float64_case(rs, b, n, m, c, widths, idx_np):
    xyz = rs.rand(b, n, 3).astype(np.float32)
    new_xyz = rs.rand(b, m, 3).astype(np.float32)
    pts = rs.randn(b, n, c).astype(np.float32)
    ws, bs, cc = [], [], 3 + c
    for w_ in widths:
        ws.append((rs.randn(cc, w_) / np.sqrt(cc)).astype(np.float32))
        bs.append((0.1 * rs.randn(w_)).astype(np.float32))
        cc = w_
    bi = np.arange(b)[:, None, None]
    g = np.concatenate([xyz[bi, idx_np] - new_xyz[:, :, None, :], pts[bi, idx_np]], -1).astype(np.float64)  # (b, m, 32, 3 + c)
    for w_, b_ in zip(ws, bs):
        g = np.maximum(g @ w_.astype(np.float64) + b_, 0.0)
    return xyz, new_xyz, pts, ws, bs, g


@pytest.mark.parametrize("hoisted", [True, False])
def test_packed_tables_match_float64(pn2, cuda, packing, hoisted):  # noqa: F811
    """the existing float64 test of this kernel draws random indices, which never pack: `mixed` tables, two chunks"""
    tfu = pn2.util.tf_util
    b, n, m, c, widths = 2, 64, 100, 64, (256, 256, 512)
    idx_np = r07._table("mixed", b * m, n, seed=5).reshape(b, m, 32)
    assert wide_tiles(idx_np) < b * m
    xyz, new_xyz, pts, ws, bs, g = _float64_case(np.random.RandomState(17), b, n, m, c, widths, idx_np)
    kws = [tfu.sa_wide_first_layer(T(ws[0], cuda))] + [T(w_, cuda) for w_ in ws[1:]]
    run = tfu.hip_sa_mlp_wide_pre if hoisted else tfu.hip_sa_mlp_wide
    packing(True, cuda)
    y = run(T(xyz, cuda), T(new_xyz, cuda), T(pts, cuda), T(idx_np, cuda), kws, [T(b_, cuda) for b_ in bs])
    assert y is not None and y.shape == (b, m, widths[-1])
    close(y.cpu().numpy(), g.max(2))


def test_unpooled_and_unaligned_idx_take_the_unpacked_kernel(pn2, cuda, packing):  # noqa: F811
    """pool = False and an idx that is not 16-byte aligned are outside PACK: same float64 bound, and the unaligned call gives the
    bits of the aligned one (which packs)"""
    tfu = pn2.util.tf_util
    b, n, m, c, widths = 2, 64, 100, 64, (128, 256)
    idx_np = r07._table("mixed", b * m, n, seed=9).reshape(b, m, 32)
    assert wide_tiles(idx_np) < b * m
    xyz, new_xyz, pts, ws, bs, g = _float64_case(np.random.RandomState(23), b, n, m, c, widths, idx_np)
    kws = [tfu.sa_wide_first_layer(T(ws[0], cuda))] + [T(w_, cuda) for w_ in ws[1:]]
    tb = [T(b_, cuda) for b_ in bs]
    packing(True, cuda)
    rows = tfu.hip_sa_mlp_wide(T(xyz, cuda), T(new_xyz, cuda), T(pts, cuda), T(idx_np, cuda), kws, tb, pool=False)
    assert rows is not None and rows.shape == g.shape
    close(rows.cpu().numpy(), g)
    shifted = torch.empty(b * m * 32 + 1, dtype=torch.int32, device=cuda)
    shifted[1:] = T(idx_np, cuda).reshape(-1)
    idx_odd = shifted[1:].reshape(b, m, 32)
    assert idx_odd.data_ptr() % 16 == 4 and idx_odd.is_contiguous()
    for run in (tfu.hip_sa_mlp_wide, tfu.hip_sa_mlp_wide_pre):
        odd = run(T(xyz, cuda), T(new_xyz, cuda), T(pts, cuda), idx_odd, kws, tb)
        even = run(T(xyz, cuda), T(new_xyz, cuda), T(pts, cuda), T(idx_np, cuda), kws, tb)
        assert odd is not None and even is not None
        close(odd.cpu().numpy(), g.max(2))
        assert torch.equal(odd, even)


def test_real_ball_query_tables_of_a_clustered_cloud(pn2, cuda, packing):  # noqa: F811
    """an SA3-like level ([128,128,256] on 128 channels, 2 x 64 centres) with the library's own sampling and ball query on a
    clustered cloud, whose short balls pack: same bits on / off, and float64"""
    tfu, pu = pn2.util.tf_util, pn2.util.pointnet_util
    b, n, m, c, widths = 2, 256, 64, 128, (128, 128, 256)
    rs = np.random.RandomState(31)
    centres = rs.uniform(-4, 4, (b, 24, 1, 3))
    xyz_np = (centres + 0.05 * rs.randn(b, 24, n // 24 + 1, 3)).reshape(b, -1, 3)[:, :n].astype(np.float32)
    with torch.no_grad():
        new_xyz, idx = pu.sa_geometry(T(xyz_np, cuda), m, 1.0, 32)
    idx_np = idx.cpu().numpy()
    tiles = wide_tiles(idx_np)
    print("clustered cloud: class shares (8, 16, 32) %.2f %.2f %.2f, %d tiles for %d groups" % (r07.class_shares(idx_np) + (tiles, b * m)))
    assert tiles <= 0.75 * b * m
    _, _, pts, ws, bs, _ = _float64_case(rs, b, n, m, c, widths, idx_np)
    new_np = new_xyz.cpu().numpy()
    bi = np.arange(b)[:, None, None]
    g = np.concatenate([xyz_np[bi, idx_np] - new_np[:, :, None, :], pts[bi, idx_np]], -1).astype(np.float64)
    for w_, b_ in zip(ws, bs):
        g = np.maximum(g @ w_.astype(np.float64) + b_, 0.0)
    kws = [tfu.sa_wide_first_layer(T(ws[0], cuda))] + [T(w_, cuda) for w_ in ws[1:]]
    tb = [T(b_, cuda) for b_ in bs]
    for run in (tfu.hip_sa_mlp_wide_pre, tfu.hip_sa_mlp_wide):
        outs = {}
        for on in (False, True):
            packing(on, cuda)
            outs[on] = run(T(xyz_np, cuda), new_xyz, T(pts, cuda), idx, kws, tb)
            assert outs[on] is not None
        assert torch.equal(outs[True], outs[False])
        close(outs[True].cpu().numpy(), g.max(2))


def _wide_kernels(run):
    """names of the mlp_wide_kernel instantiations `run` launches (torch profiler, as tests/test_in_place_gpu.py reads them)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "mlp_wide_kernel" in e.name}
    assert names, "the profiler saw no mlp_wide_kernel"
    return names


def test_the_switch_selects_the_packed_instantiation(pn2, cuda, packing):  # noqa: F811
    """the on / off comparisons above would also pass if the launcher never chose PACK: the kernel that runs is
    mlp_wide_kernel<1, true> with the switch on (pooled, aligned idx) and <1, false> with it off, un-pooled, or unaligned"""
    tfu = pn2.util.tf_util
    b, n, m, c, widths = 2, 64, 100, 64, (128, 256)
    idx_np = r07._table("mixed", b * m, n, seed=9).reshape(b, m, 32)
    xyz, new_xyz, pts, ws, bs, _ = _float64_case(np.random.RandomState(29), b, n, m, c, widths, idx_np)
    kws = [tfu.sa_wide_first_layer(T(ws[0], cuda))] + [T(w_, cuda) for w_ in ws[1:]]
    tb = [T(b_, cuda) for b_ in bs]
    txyz, tnew, tpts, tidx = T(xyz, cuda), T(new_xyz, cuda), T(pts, cuda), T(idx_np, cuda)
    shifted = torch.empty(b * m * 32 + 1, dtype=torch.int32, device=cuda)
    shifted[1:] = tidx.reshape(-1)
    idx_odd = shifted[1:].reshape(b, m, 32)

    def packed(names):
        assert len(names) == 1, names
        name = next(iter(names)).replace(" ", "")  # demangled, or the mangled template arguments
        on_ = "mlp_wide_kernel<1,true>" in name or "mlp_wide_kernelILi1ELb1EE" in name
        off_ = "mlp_wide_kernel<1,false>" in name or "mlp_wide_kernelILi1ELb0EE" in name
        assert on_ != off_, name
        return on_

    for run in (tfu.hip_sa_mlp_wide, tfu.hip_sa_mlp_wide_pre):
        if run is tfu.hip_sa_mlp_wide_pre:
            run(txyz, tnew, tpts, tidx, kws, tb)  # the hoisted product's own launch may be a (plain) wide kernel: keep only mode 1
        only1 = lambda names: {nm for nm in names if "mlp_wide_kernel<1" in nm.replace(" ", "") or "mlp_wide_kernelILi1E" in nm}  # noqa: E731
        packing(True, cuda)
        assert packed(only1(_wide_kernels(lambda: run(txyz, tnew, tpts, tidx, kws, tb))))
        assert not packed(only1(_wide_kernels(lambda: run(txyz, tnew, tpts, idx_odd, kws, tb))))
        assert not packed(only1(_wide_kernels(lambda: run(txyz, tnew, tpts, tidx, kws, tb, pool=False))))
        packing(False, cuda)
        assert not packed(only1(_wide_kernels(lambda: run(txyz, tnew, tpts, tidx, kws, tb))))
