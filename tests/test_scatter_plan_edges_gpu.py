"""The scatter plan behind the seven gradients of a training step's backward pass (pn2_scatter_plan_build, _build_multi, _apply and
the two *_grad_ws doors, csrc/pn2_interpolate.hip) at its edges, through the C ABI, against the numpy reference of
tests/scatter_ref.py (itself checked by tests/test_scatter_plan_edges_cpu.py).

Shapes come from the kernels: the gather maps a thread to (source slot, float4 column) with spb = 256 // (c / 4) sources per block
and walks a list four entries at a time; the three-kernel build scans with 256 threads, the one-launch build with 1024 and LDS
counters for up to 16384 sources.  Every output, plan and plan buffer is a view inside a tensor filled with a NaN bit pattern, a
plan view exactly pn2_scatter_plan_bytes long: what a call writes outside its view, or leaves unwritten inside an output, fails.

Two kinds of assertion.  EXACT: on scatter_ref.exact_data the float32 result is the same in any summation order and equals the
float64 reference bit for bit, so everything structural (a dropped, doubled or misplaced entry, a wrong offset, a weight that is
not the forward's) changes bits; plans are decoded and checked entry by entry (scatter_ref.check_plan).  BOUND: on normal data,
elementwise |err| <= (L + 2) 2^-24 sum_abs (scatter_ref.bound: the worst case of a length-L fma chain in any order; derived, not
measured).  Every test prints a "[scatter_edges]" line (pytest -s); the general-data ones give the worst err / bound."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scatter_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5B                 # int32 of 0xFFA5A5A5: a NaN as float32
LEAD = 64                          # margin, in 4-byte words, on both sides of every view
OK, EINVAL, ENULL, EUNSUP = 0, -1, -2, -4


# ------------------------------------------------------------------------------------------------------- guarded buffers
class Buf:
    """`n` 4-byte words inside a larger poisoned tensor, `off` words past a 16-byte boundary; data: a float32 / int32 array"""

    def __init__(self, dev, n, data=None, off=0):
        import torch
        self.n, self.lead = int(n), LEAD + off
        self.base = torch.full((self.lead + self.n + LEAD,), POISON, dtype=torch.int32, device=dev)
        self.t = self.base[self.lead:self.lead + self.n]
        assert self.t.data_ptr() % 16 == (4 * off) % 16
        self.init = None
        if data is not None:
            self.set(data)

    def set(self, data):
        import torch
        a = np.ascontiguousarray(data)
        assert a.dtype.itemsize == 4 and a.size == self.n
        self.init = a.reshape(-1).view(np.int32).copy()
        self.t.copy_(torch.from_numpy(self.init))

    def ptr(self, byte_offset=0):
        return ctypes.c_void_p(self.t.data_ptr() + byte_offset)

    def words(self):
        """the view's words after checking that both margins still hold the poison"""
        b = self.base.cpu().numpy()
        assert (b[:self.lead] == POISON).all() and (b[self.lead + self.n:] == POISON).all(), "wrote outside its view"
        return b[self.lead:self.lead + self.n]

    def f32(self, shape):
        return self.words().view(np.float32).reshape(shape).copy()

    def untouched(self):
        w = self.words()
        return bool((w == POISON).all()) if self.init is None else np.array_equal(w, self.init)


def sync():
    import torch
    torch.cuda.synchronize()


def same_bits(a, b):
    return np.array_equal(S.bits(a), S.bits(b))


def assert_bits(got, ref64, what):
    want = np.asarray(ref64).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref64), "the reference of %s is not a float32 number" % what
    bad = S.bits(got) != S.bits(want)
    assert not bad.any(), "%s: %d of %d elements differ from float64, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


class Case:
    """idx / weight operand of one build on the device, with the host's copy"""

    def __init__(self, dev, idx, wdata, kind, div, nsrc):
        self.b, self.nent = idx.shape
        self.idx, self.wdata, self.kind, self.div, self.nsrc = idx, wdata, kind, div, nsrc
        self.w32 = S.entry_weights(self.b, self.nent, kind, wdata)
        self.d_idx = Buf(dev, idx.size, idx.astype(np.int32))
        self.d_w = None if kind == 0 else Buf(dev, np.size(wdata), S.f32(wdata))
        self.words = S.plan_words(self.b, self.nent, nsrc)

    def inputs_untouched(self):
        return self.d_idx.untouched() and (self.d_w is None or self.d_w.untouched())

    def check(self, plan_words):
        S.check_plan(*S.decode_plan(np.ascontiguousarray(plan_words), self.b, self.nent, self.nsrc), self.idx, self.w32, self.div, self.nsrc)


def build_single(raw, dev, cs, off=0, expect=OK, **over):
    """pn2_scatter_plan_build into a poisoned view of exactly pn2_scatter_plan_bytes -> the plan Buf (checked unless refused)"""
    nbytes = int(raw.pn2_scatter_plan_bytes(cs.b, cs.nent, cs.nsrc))
    assert nbytes == 4 * cs.words
    plan = Buf(dev, cs.words, off=off)
    a = dict(b=cs.b, nent=cs.nent, div=cs.div, nsrc=cs.nsrc, idx=cs.d_idx.ptr(), w=None if cs.d_w is None else cs.d_w.ptr(),
             kind=cs.kind, plan=plan.ptr(), bytes=nbytes)
    a.update(over)
    rc = raw.pn2_scatter_plan_build(a["b"], a["nent"], a["div"], a["nsrc"], a["idx"], a["w"], a["kind"], a["plan"], a["bytes"], None)
    sync()
    assert rc == expect, "pn2_scatter_plan_build returned %d, expected %d (%s)" % (rc, expect, over)
    assert cs.inputs_untouched()
    if expect != OK:
        assert plan.untouched(), "the build refused the call (%d) but wrote to the plan" % rc
    else:
        cs.check(plan.words())
    return plan


def apply_plan(raw, dev, cs, pbuf, rows, c, in_stride=None, row_off=0, expect=OK, out_off=0, **over):
    """pn2_scatter_plan_apply of rows (b, nent // div, c) laid out `in_stride` floats apart, starting row_off floats past a
    16-byte boundary, NaN poison in the columns outside the slice, into a poisoned out -> out (b, nsrc, c) float32"""
    in_stride = c if in_stride is None else in_stride
    n = cs.nent // cs.div
    wide = np.full((cs.b, n, max(in_stride, c)), POISON, np.int32)
    wide[:, :, :c] = S.f32(rows).view(np.int32)
    d_rows = Buf(dev, wide.size, wide, off=row_off)
    out = Buf(dev, cs.b * cs.nsrc * c, off=out_off)
    a = dict(b=cs.b, nent=cs.nent, div=cs.div, c=c, nsrc=cs.nsrc, rows=d_rows.ptr(), stride=in_stride, plan=pbuf.ptr(), bytes=4 * cs.words,
             out=out.ptr())
    a.update(over)
    rc = raw.pn2_scatter_plan_apply(a["b"], a["nent"], a["div"], a["c"], a["nsrc"], a["rows"], a["stride"], a["plan"], a["bytes"],
                                    a["out"], None)
    sync()
    assert rc == expect, "pn2_scatter_plan_apply returned %d, expected %d (%s)" % (rc, expect, over)
    assert d_rows.untouched() and pbuf.words() is not None
    if expect != OK:
        assert out.untouched(), "the apply refused the call (%d) but wrote to out" % rc
        return None
    return out.f32((cs.b, cs.nsrc, c))


def within_bound(got, ref, sum_abs, L, what):
    """elementwise |got - ref| <= (L + 2) 2^-24 sum_abs -> worst err / bound"""
    err, bd = np.abs(got.astype(np.float64) - ref), S.bound(sum_abs, L)
    assert np.isfinite(got).all(), "%s: not finite" % what
    ratio = float((err[bd > 0] / bd[bd > 0]).max()) if (bd > 0).any() else 0.0
    assert (err <= bd).all(), "%s: %d elements outside the bound, worst err / bound %.3g (empty lists must give 0: %s)" % (
        what, int((err > bd).sum()), ratio, bool((err[bd == 0] == 0).all()))
    return ratio


# ======================================================================================== 1. apply: the column sweep, exact
@pytest.mark.parametrize("c", S.APPLY_C)
def test_apply_column_sweep_exact(pn2, cuda, c):
    """c in {4, 8, 12, 20, 36, 132, 260, 512, 516, 1020, 1024} (c / 4 divides 256, leaves idle threads, one source per block) x
    nsrc in {1, spb - 1, spb, spb + 1, 3 spb + 1} x b in {1, 3} x (div 1 / kind 0, div 3 / kinds 1 and 2): single build + apply on
    exact data, bit-equal to float64; the plan decoded and checked; out poisoned beforehand (empty sources come back as zeros)."""
    raw = pn2._lib._raw
    n = 0
    for cc, nsrc, b, div, kind in S.apply_cases():
        if cc != c:
            continue
        idx, rows, wdata, w32 = S.apply_case(c, nsrc, b, div, kind)
        cs = Case(cuda, idx, wdata, kind, div, nsrc)
        plan = build_single(raw, cuda, cs)
        got = apply_plan(raw, cuda, cs, plan, rows, c)
        ref, _, L = S.scatter_f64(idx, rows, w32, div, nsrc)
        assert_bits(got, ref, "c=%d nsrc=%d b=%d div=%d kind=%d" % (c, nsrc, b, div, kind))
        assert not got[L == 0].any()
        n += 1
    print("[scatter_edges] apply sweep c=%d: %d cases bit-equal to float64 (nsrc %s)" % (c, n, S.apply_nsrc(c)))


# ================================================================================ 2. apply: operand layout, plan position
@pytest.mark.parametrize("c", [4, 36, 260, 1024])
def test_apply_operand_layout_and_plan_position(pn2, cuda, c):
    """in_stride in {c, c + 4, c + 3} x rows_in starting 0 and 3 floats past a 16-byte boundary (the aligned template with a column
    slice; the unaligned one), NaN poison in the columns outside the slice; and the plan copied to a view that is 4-byte but not
    16-byte aligned: the same bits as float64 every time."""
    raw = pn2._lib._raw
    nsrc, b = S.spb(c) + 1, 3
    for div, kind in S.MODES:
        idx, rows, wdata, w32 = S.apply_case(c, nsrc, b, div, kind)
        cs = Case(cuda, idx, wdata, kind, div, nsrc)
        plan = build_single(raw, cuda, cs)
        ref = S.scatter_f64(idx, rows, w32, div, nsrc)[0]
        for stride in (c, c + 4, c + 3):
            for row_off in (0, 3):
                got = apply_plan(raw, cuda, cs, plan, rows, c, in_stride=stride, row_off=row_off)
                assert_bits(got, ref, "c=%d kind=%d in_stride=%d rows_in +%d floats" % (c, kind, stride, row_off))
        for off in (1, 3):
            moved = Buf(cuda, cs.words, plan.words(), off=off)
            assert moved.t.data_ptr() % 16 != 0
            got = apply_plan(raw, cuda, cs, moved, rows, c, in_stride=c + 4)
            assert_bits(got, ref, "c=%d kind=%d plan copied to +%d words" % (c, kind, off))
            assert moved.untouched()
    print("[scatter_edges] apply layout c=%d: 3 strides x 2 row offsets x 3 kinds + 2 plan copies bit-equal to float64" % c)


# ================================================================================================ 3. the single build
@pytest.mark.parametrize("nsrc", S.BUILD_NSRC)
def test_single_build_exact(pn2, cuda, nsrc):
    """nsrc in {1, 2, 255, 256, 257, 511, 513} (the 256-thread scan: one counter per thread, the first thread with two, an idle
    tail) x nent in {1, 255, 256, 257} x div, kinds 0 / 1 / 2, b = 2: the decoded plan entry by entry (kind 2: the weights
    bit-equal to scatter_ref.weights_f32), then apply (c = 4) bit-equal to float64."""
    raw = pn2._lib._raw
    n = 0
    for case in S.build_cases():
        if case[1] != nsrc or case[0] != 2:
            continue
        b, _, nrows, div, kind = case
        idx, rows, wdata, w32 = S.build_case(*case)
        cs = Case(cuda, idx, wdata, kind, div, nsrc)
        plan = build_single(raw, cuda, cs, off=n % 4)              # a plan is 4-byte aligned, no more
        got = apply_plan(raw, cuda, cs, plan, rows, 4)
        assert_bits(got, S.scatter_f64(idx, rows, w32, div, nsrc)[0], "nsrc=%d nent=%d kind=%d" % (nsrc, nrows * div, kind))
        n += 1
    assert n == 12
    print("[scatter_edges] single build nsrc=%d: %d plans valid, applies bit-equal to float64" % (nsrc, n))


@pytest.mark.parametrize("div,kind", S.MODES)
def test_single_build_grid_stride(pn2, cuda, div, kind):
    """b = 64, nsrc = 257, nent = 8192 + 257 (rounded up to whole rows): the count and fill grids are capped at ceil(2048 / 64) = 32
    blocks of 256, so every thread takes a second entry and 257 of them a third."""
    raw = pn2._lib._raw
    case = [cs for cs in S.build_cases() if cs[0] == 64 and cs[4] == kind][0]
    assert case[2] * div >= 8192 + 257 > 32 * 256
    idx, rows, wdata, w32 = S.build_case(*case)
    cs = Case(cuda, idx, wdata, kind, div, 257)
    plan = build_single(raw, cuda, cs)
    got = apply_plan(raw, cuda, cs, plan, rows, 4)
    assert_bits(got, S.scatter_f64(idx, rows, w32, div, 257)[0], "grid stride kind=%d" % kind)
    print("[scatter_edges] single build grid stride kind=%d: b=64 nsrc=257 nent=%d valid, apply bit-equal" % (kind, cs.nent))


# ================================================================================================= 4. the multi build
def build_multi(raw, dev, cases, extra_gap=True, expect=OK, **over):
    """pn2_scatter_plan_build_multi into ONE poisoned buffer: plan i at a 16-byte-rounded offset, the first 16 bytes in, every other
    slice 16 bytes further than it must be -> (buffer Buf, word offsets)"""
    b = cases[0].b
    offs, total = [], 16
    for i, cs in enumerate(cases):
        offs.append(total)
        total += (4 * cs.words + 15) // 16 * 16 + (16 if extra_gap and i % 2 else 0)
    buf = Buf(dev, total // 4)
    n = len(cases)
    arr = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    a = dict(nplans=n, b=b, nent=arr([cs.nent for cs in cases]), div=arr([cs.div for cs in cases]), nsrc=arr([cs.nsrc for cs in cases]),
             idx=(ctypes.c_void_p * n)(*[cs.d_idx.t.data_ptr() for cs in cases]),
             w=(ctypes.c_void_p * n)(*[None if cs.d_w is None else cs.d_w.t.data_ptr() for cs in cases]),
             kind=arr([cs.kind for cs in cases]), buffer=buf.ptr(), offset=(ctypes.c_uint64 * n)(*offs), bytes=total)
    a.update(over)
    rc = raw.pn2_scatter_plan_build_multi(a["nplans"], a["b"], a["nent"], a["div"], a["nsrc"], a["idx"], a["w"], a["kind"], a["buffer"],
                                          a["offset"], a["bytes"], None)
    sync()
    assert rc == expect, "pn2_scatter_plan_build_multi returned %d, expected %d (%s)" % (rc, expect, sorted(over))
    assert all(cs.inputs_untouched() for cs in cases)
    if expect != OK:
        assert buf.untouched(), "the multi build refused the call (%d) but wrote to the buffer" % rc
    return buf, [o // 4 for o in offs]


def check_multi(raw, dev, name):
    b = S.MULTI_B[name]
    specs = S.multi_specs(name)
    data = [S.multi_case(name, i) for i in range(len(specs))]
    cases = [Case(dev, d[0], d[2], sp[3], sp[2], sp[0]) for d, sp in zip(data, specs)]
    buf, offs = build_multi(raw, dev, cases)
    words = buf.words()                                            # (checks the outer margins)
    covered = np.zeros(buf.n, bool)
    for cs, o in zip(cases, offs):
        covered[o:o + cs.words] = True
        cs.check(words[o:o + cs.words])
    lds = max(sp[0] for sp in specs) <= 16384
    if lds:     # nothing but the plans is written: the padding up to 16 bytes, the gaps and the head of the buffer are still poison
        assert (~covered).sum() >= 4 and (words[~covered] == POISON).all(), "the one-launch build wrote between the plan slices"
    else:       # one memset of offset[0] .. end: only what lies in front of it is still poison
        assert (words[:offs[0]] == POISON).all()
    for i, (cs, o, d) in enumerate(zip(cases, offs, data)):
        idx, rows, _, w32 = d
        ref = S.scatter_f64(idx, rows, w32, cs.div, cs.nsrc)[0]
        single = build_single(raw, dev, cs)
        copied = Buf(dev, cs.words, words[o:o + cs.words], off=i % 4)
        got = apply_plan(raw, dev, cs, copied, rows, 4)
        assert same_bits(got, apply_plan(raw, dev, cs, single, rows, 4)), "%s plan %d: the apply differs from the single build's" % (name, cs.nsrc)
        assert_bits(got, ref, "%s nsrc=%d kind=%d" % (name, cs.nsrc, cs.kind))
    print("[scatter_edges] multi build %s (%s path, b=%d): %d plans valid, applies bit-equal to the single builds' and to float64" % (
        name, "LDS" if lds else "global", b, len(cases)))
    return buf, offs, cases


@pytest.mark.parametrize("name", [k for k in S.MULTI_BATCHES if k.startswith("lds")])
def test_multi_build_lds_path(pn2, cuda, name):
    """nsrc in {1, 63, 64, 65, 1023, 1024, 1025, 2049, 16384} mixed in one call (the dynamic LDS is sized by the largest plan, each
    plan splits it at its own nsrc), nplans in {1, 8}, kinds 0 / 1 / 2 mixed: every plan decoded and checked, its apply bit-equal to
    the single build's apply and to float64, and every word of the buffer outside the plans -- the padding after a plan that ends
    8 bytes off a 16-byte boundary, 16-byte gaps, the head -- still poison."""
    check_multi(pn2._lib._raw, cuda, name)


def test_multi_build_global_path(pn2, cuda):
    """the lds8_max batch with 16385 sources in one plan: one source too many for LDS sends the whole batch through the memset and
    the three launches.  Same checks; of the poison only what lies outside offset[0] .. end."""
    check_multi(pn2._lib._raw, cuda, "global8")


def test_multi_build_in_place_apply(pn2, cuda):
    """a plan applied where the multi build left it (no copy): slices of one buffer at 16-byte-rounded offsets, as the training step
    uses them"""
    raw = pn2._lib._raw
    specs = S.multi_specs("lds8")
    data = [S.multi_case("lds8", i, c=8) for i in range(len(specs))]
    cases = [Case(cuda, d[0], d[2], sp[3], sp[2], sp[0]) for d, sp in zip(data, specs)]
    buf, offs = build_multi(raw, cuda, cases)
    before = buf.words().copy()
    for cs, o, d in zip(cases, offs, data):
        got = apply_plan(raw, cuda, cs, buf, d[1], 8, plan=buf.ptr(4 * o))
        assert_bits(got, S.scatter_f64(d[0], d[1], d[3], cs.div, cs.nsrc)[0], "in place nsrc=%d" % cs.nsrc)
    assert np.array_equal(buf.words(), before), "an apply wrote to its plan"
    print("[scatter_edges] multi build, plans applied in place: %d bit-equal to float64" % len(cases))


def test_python_wrapper_chunks_at_eight(pn2, cuda):
    """util.pointnet_util.scatter_plans with 9 live specs and interleaved Nones (two calls of pn2_scatter_plan_build_multi: 8 + 1):
    None passes through, every plan has pn2_scatter_plan_bytes bytes, decodes to a valid plan and applies (through
    _scatter_plan_apply) bit-equal to float64."""
    import torch
    pu = pn2.util.pointnet_util
    b = 2
    shapes = [(1, 0), None, (63, 1), (64, 2), None, None, (65, 0), (257, 1), (1023, 2), (1024, 0), None, (1025, 1), (300, 2), None]
    specs, keep = [], []
    for i, sh in enumerate(shapes):
        if sh is None:
            specs.append(None)
            keep.append(None)
            continue
        nsrc, kind = sh
        div = 1 if kind == 0 else 3
        nrows = S.multi_rows(nsrc, div)
        idx = S.make_idx(b, nsrc, nrows, div, 100 + i, phase=i)
        rows, wdata = S.exact_data(idx, div, 8, kind, 200 + i)
        k = 32 if kind == 0 else 3                                  # the wrapper takes idx as (b, rows, k): k = div with weights
        pad = (-idx.shape[1]) % k
        assert pad == 0 or kind == 0
        if pad:                                                     # whole groups of 32 for the grouping form
            idx = np.concatenate([idx, idx[:, :pad]], axis=1)
            rows = np.concatenate([rows, rows[:, :pad]], axis=1)
        t_idx = torch.from_numpy(idx.reshape(b, -1, k)).to(cuda)
        t_w = None if kind == 0 else torch.from_numpy(S.f32(wdata).reshape(b, -1, 3)).to(cuda)
        specs.append((t_idx, nsrc, t_w, kind if kind else None))
        keep.append((idx, rows, wdata, kind, div, nsrc))
    assert sum(s is not None for s in specs) == 9
    pn2._lib.lib.trace = calls = []
    try:
        plans = pu.scatter_plans(specs)
        torch.cuda.synchronize()
    finally:
        pn2._lib.lib.trace = None
    assert [t[0] for t in calls] == ["pn2_scatter_plan_build_multi"] * 2 and [t[1][0] for t in calls] == [8, 1]
    assert len(plans) == len(specs)
    for sp, kp, plan in zip(specs, keep, plans):
        if sp is None:
            assert plan is None
            continue
        idx, rows, wdata, kind, div, nsrc = kp
        nent = idx.shape[1]
        w32 = S.entry_weights(b, nent, kind, wdata)
        assert plan.numel() == pn2._lib._raw.pn2_scatter_plan_bytes(b, nent, nsrc) and plan.data_ptr() % 16 == 0
        S.check_plan(*S.decode_plan(plan.cpu().numpy(), b, nent, nsrc), idx, w32, div, nsrc)
        g = torch.from_numpy(rows).to(cuda)
        got = pu._scatter_plan_apply(plan, g, 0, 8, nent, div, nsrc).cpu().numpy()
        assert_bits(got, S.scatter_f64(idx, rows, w32, div, nsrc)[0], "wrapper nsrc=%d kind=%d" % (nsrc, kind))
    print("[scatter_edges] scatter_plans: 9 live specs in 2 calls (8 + 1), 5 Nones passed through, all plans valid and bit-equal")


# ================================================================================= 5. forward / backward weight agreement
@pytest.mark.parametrize("c1", [0, 16])
def test_plan_weights_are_the_forwards_weights(pn2, cuda, c1):
    """m = c2 = 16, points2 = identity rows, idx rows without repeats: pn2_fp_interp_concat writes the forward's three weights of a
    row at the columns idx (c1 = 0: the row kernels; c1 = 16: the 16-byte-lane kernel).  Distances: general positive floats, rows
    with one and with two zeros (the 1e-10 clamp).  The forward's weights, the plan's weights
    for the same (dist, idx) from the single and from the multi build, and scatter_ref.weights_f32 are all bit-equal."""
    raw = pn2._lib._raw
    b, n, m = 2, 200, 16
    rs = np.random.RandomState(16 + c1)
    idx = np.stack([np.stack([rs.permutation(m)[:3] for _ in range(n)]) for _ in range(b)]).astype(np.int32)
    dist = (10.0 ** rs.uniform(-5, 3, (b, n, 3))).astype(np.float32)
    dist[:, 3::10, 0] = 0.0
    dist[:, 5::10, 2] = 0.0
    dist[:, 7::10, :2] = 0.0
    dist[:, 8::10, 1:] = 0.0
    w = S.weights_f32(dist)
    p2 = np.tile(np.eye(m, dtype=np.float32), (b, 1, 1))
    p1 = rs.randn(b, n, c1).astype(np.float32) if c1 else None
    d_dist, d_idx, d_p2 = Buf(cuda, dist.size, dist), Buf(cuda, idx.size, idx), Buf(cuda, p2.size, p2)
    d_p1 = Buf(cuda, p1.size, p1) if c1 else None
    out = Buf(cuda, b * n * (m + c1))
    rc = raw.pn2_fp_interp_concat(b, n, m, c1, m, d_dist.ptr(), d_idx.ptr(), None if d_p1 is None else d_p1.ptr(), d_p2.ptr(), out.ptr(),
                                  m + c1, None)
    sync()
    assert rc == OK
    fwd = out.f32((b, n, m + c1))
    want = np.zeros((b, n, m), np.float32)
    np.put_along_axis(want, idx.astype(np.int64), w, axis=2)
    assert same_bits(fwd[:, :, :m], want), "the forward's weights differ from the float32 restatement"
    assert c1 == 0 or same_bits(fwd[:, :, m:], p1)
    w_fwd = np.take_along_axis(fwd[:, :, :m], idx.astype(np.int64), axis=2).reshape(b, 3 * n)
    cs = Case(cuda, idx.reshape(b, 3 * n), dist, 2, 3, m)
    assert same_bits(cs.w32, w_fwd)
    cs.w32 = w_fwd                                                  # hold the plans to the forward's own output
    build_single(raw, cuda, cs)
    buf, offs = build_multi(raw, cuda, [cs])
    cs.check(buf.words()[offs[0]:offs[0] + cs.words])
    print("[scatter_edges] forward / backward weights c1=%d: %d weights bit-equal (forward, single build, multi build, restatement)" % (
        c1, w.size))


# ======================================================================================================== 6. general data
@pytest.mark.parametrize("case", S.GENERAL_CASES, ids=lambda v: "c%d-nsrc%d-b%d-div%d-kind%d" % v)
def test_general_data_within_the_derived_bound(pn2, cuda, case):
    """normal rows, random weights / distances (kind 2: every fifth row with one clamped distance, every seventh with two), one per
    c class, each with a hot source: single build + apply and the LDS multi build + apply, elementwise
    |err| <= (L + 2) 2^-24 sum_abs against float64 with the float32 weights of scatter_ref.weights_f32; in_stride = c + 4."""
    raw = pn2._lib._raw
    c, nsrc, b, div, kind = case
    idx, rows, wdata, w32 = S.apply_case(c, nsrc, b, div, kind, exact=False)
    ref, sa, L = S.scatter_f64(idx, rows, w32, div, nsrc)
    cs = Case(cuda, idx, wdata, kind, div, nsrc)
    plan = build_single(raw, cuda, cs)
    r1 = within_bound(apply_plan(raw, cuda, cs, plan, rows, c, in_stride=c + 4), ref, sa, L, "single build")
    buf, offs = build_multi(raw, cuda, [cs])
    cs.check(buf.words()[offs[0]:offs[0] + cs.words])
    r2 = within_bound(apply_plan(raw, cuda, cs, buf, rows, c, plan=buf.ptr(4 * offs[0])), ref, sa, L, "multi build")
    print("[scatter_edges] general c=%d nsrc=%d b=%d div=%d kind=%d: longest list %d, worst err/bound %.3g (single build) %.3g (multi)" % (
        case + (int(L.max()), r1, r2)))


# ============================================================================================================ 7. the doors
def test_three_interpolate_grad_ws_door(pn2, cuda):
    """pn2_three_interpolate_grad_ws switches from float atomics to the list path at b n 3 c >= 2^20: b = 1, c = 128, n = 2730
    (1048320: atomics, the workspace stays untouched) and n = 2731 (1048704: the list path, the workspace holds a valid plan).
    Exact data: both bit-equal to float64.  Called through the traced proxy: the trace names the entry point."""
    raw, lib = pn2._lib._raw, pn2._lib.lib
    b, c, m = 1, 128, 37
    for n, listed in ((2730, False), (2731, True)):
        assert (b * n * 3 * c >= 1 << 20) == listed
        idx = S.make_idx(b, m, n, 3, n)
        rows, w = S.exact_data(idx, 3, c, 1, n + 1)
        d_g, d_idx, d_w = Buf(cuda, rows.size, rows), Buf(cuda, idx.size, idx), Buf(cuda, w.size, w)
        nbytes = int(raw.pn2_three_interpolate_grad_workspace_bytes(b, n, m))
        assert nbytes == 4 * S.plan_words(b, 3 * n, m)
        ws, out = Buf(cuda, nbytes // 4), Buf(cuda, b * m * c)
        lib.trace = calls = []
        try:
            rc = lib.pn2_three_interpolate_grad_ws(b, n, c, m, d_g.ptr(), d_idx.ptr(), d_w.ptr(), out.ptr(), ws.ptr(), nbytes, None)
        finally:
            lib.trace = None
        sync()
        assert rc == OK and [t[0] for t in calls] == ["pn2_three_interpolate_grad_ws"]
        assert d_g.untouched() and d_idx.untouched() and d_w.untouched()
        assert_bits(out.f32((b, m, c)), S.scatter_f64(idx, rows, w, 3, m)[0], "three_interpolate_grad_ws n=%d" % n)
        if listed:
            S.check_plan(*S.decode_plan(ws.words(), b, 3 * n, m), idx, w, 3, m)
        else:
            assert ws.untouched(), "below the threshold the workspace is not used"
    print("[scatter_edges] pn2_three_interpolate_grad_ws: atomics at n=2730, list path at n=2731, both bit-equal to float64")


def test_group_point_grad_ws_door(pn2, cuda):
    """pn2_group_point_grad_ws takes the list path from b m nsample c >= 2^20 (csrc/pn2_grouping.hip): b = 1, c = 128, nsample = 8,
    m = 1023 (atomics) and m = 1024 (exactly 2^20: the list path).  Same checks."""
    raw, lib = pn2._lib._raw, pn2._lib.lib
    b, c, ns, n = 1, 128, 8, 50
    for m, listed in ((1023, False), (1024, True)):
        assert (b * m * ns * c >= 1 << 20) == listed
        idx = S.make_idx(b, n, m * ns, 1, m)
        rows, _ = S.exact_data(idx, 1, c, 0, m + 1)
        d_g, d_idx = Buf(cuda, rows.size, rows), Buf(cuda, idx.size, idx)
        nbytes = int(raw.pn2_group_point_grad_workspace_bytes(b, n, m, ns))
        assert nbytes == 4 * S.plan_words(b, m * ns, n)
        ws, out = Buf(cuda, nbytes // 4), Buf(cuda, b * n * c)
        lib.trace = calls = []
        try:
            rc = lib.pn2_group_point_grad_ws(b, n, c, m, ns, d_g.ptr(), d_idx.ptr(), out.ptr(), ws.ptr(), nbytes, None)
        finally:
            lib.trace = None
        sync()
        assert rc == OK and [t[0] for t in calls] == ["pn2_group_point_grad_ws"]
        assert d_g.untouched() and d_idx.untouched()
        assert_bits(out.f32((b, n, c)), S.scatter_f64(idx, rows, None, 1, n)[0], "group_point_grad_ws m=%d" % m)
        if listed:
            S.check_plan(*S.decode_plan(ws.words(), b, m * ns, n), idx, np.ones((b, m * ns), np.float32), 1, n)
        else:
            assert ws.untouched(), "below the threshold the workspace is not used"
    print("[scatter_edges] pn2_group_point_grad_ws: atomics at m=1023, list path at m=1024, both bit-equal to float64")


# ============================================================================================================ 8. contracts
def test_argument_contracts(pn2, cuda):
    """return code, then nothing written: apply (c % 4 != 0, c = 1028, out 4 bytes off: PN2_EUNSUP; in_stride < c, plan_bytes one
    short: PN2_EINVAL), build (nent % div != 0, kind 2 with div != 3: PN2_EINVAL; kind 1 with NULL weight: PN2_ENULL), multi
    (nplans 0 / 9, an offset that is no multiple of 16, overlapping offsets, buffer_bytes one short: PN2_EINVAL); and
    pn2_scatter_plan_bytes = 4 (2 b nsrc + 2 b nent), 0 for a non-positive argument."""
    raw = pn2._lib._raw
    assert raw.pn2_scatter_plan_bytes(3, 10, 7) == 4 * (2 * 3 * 7 + 2 * 3 * 10) and raw.pn2_scatter_plan_bytes(64, 8449, 257) == 4 * 2 * 64 * 8706
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5), (2, -3, 4), (2, 3, -4)):
        assert raw.pn2_scatter_plan_bytes(*bad) == 0
    b, nsrc, c = 2, 9, 8
    idx = S.make_idx(b, nsrc, 12, 3, 1)
    rows, w = S.exact_data(idx, 3, c, 1, 2)
    cs = Case(cuda, idx, w, 1, 3, nsrc)
    plan = build_single(raw, cuda, cs)
    # apply
    for cc in (6, 1028):
        wide = np.zeros((b, 12, cc), np.float32)
        apply_plan(raw, cuda, cs, plan, wide, cc, expect=EUNSUP)
    apply_plan(raw, cuda, cs, plan, rows, c, out_off=1, expect=EUNSUP)
    apply_plan(raw, cuda, cs, plan, rows, c, expect=EINVAL, stride=c - 1)
    apply_plan(raw, cuda, cs, plan, rows, c, expect=EINVAL, bytes=4 * cs.words - 1)
    assert_bits(apply_plan(raw, cuda, cs, plan, rows, c), S.scatter_f64(idx, rows, w, 3, nsrc)[0], "the plan after the refusals")
    # build
    build_single(raw, cuda, cs, expect=EINVAL, nent=cs.nent - 1)
    build_single(raw, cuda, cs, expect=EINVAL, kind=2, div=2, nent=cs.nent)
    build_single(raw, cuda, cs, expect=EINVAL, kind=2, div=1)
    build_single(raw, cuda, cs, expect=ENULL, w=None)
    build_single(raw, cuda, cs, expect=EINVAL, bytes=4 * cs.words - 1)
    # multi
    two = [cs, Case(cuda, idx, None, 0, 1, nsrc)]
    build_multi(raw, cuda, two, expect=EINVAL, nplans=0)
    build_multi(raw, cuda, two, expect=EINVAL, nplans=9)
    good = build_multi(raw, cuda, two, extra_gap=False)
    offs = [4 * o for o in good[1]]
    total = 4 * good[0].n
    build_multi(raw, cuda, two, extra_gap=False, expect=EINVAL, offset=(ctypes.c_uint64 * 2)(offs[0], offs[1] + 8))
    build_multi(raw, cuda, two, extra_gap=False, expect=EINVAL, offset=(ctypes.c_uint64 * 2)(offs[0], offs[1] - 16))
    build_multi(raw, cuda, two, extra_gap=False, expect=EINVAL, offset=(ctypes.c_uint64 * 2)(offs[1], offs[0]))
    assert total == offs[1] + (4 * two[1].words + 15) // 16 * 16 and (4 * two[1].words) % 16 == 0
    build_multi(raw, cuda, two, extra_gap=False, expect=EINVAL, bytes=total - 1)
    print("[scatter_edges] contracts: 5 apply, 5 build, 6 multi refusals with nothing written; pn2_scatter_plan_bytes as documented")


# ========================================================================================================== 9. two devices
def test_lds_limit_on_a_second_device(pn2, cuda):
    """pn2_scatter_plan_build_multi raises the one-launch kernel's dynamic-LDS limit (128 KiB at 16384 sources); in one process the
    batch with 16384 sources is built on device 0, then on device 1: PN2_OK and valid plans on both."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    raw = pn2._lib._raw
    for dev in (torch.device("cuda:0"), torch.device("cuda:1")):
        with torch.cuda.device(dev):
            check_multi(raw, dev, "lds1_max")
            torch.cuda.synchronize()
