"""Plain numpy reference of the scatter plan (pn2_scatter_plan_build / _build_multi / _apply, csrc/pn2_interpolate.hip) and the
inputs and shapes of tests/test_scatter_plan_edges_gpu.py; held to account without a GPU by tests/test_scatter_plan_edges_cpu.py.

    out[b, idx[b, e], :] += w[b, e] * rows[b, e // div, :]        e < nent, div entries per input row

Two kinds of data.  exact_data: rows of small integers and weights from {0, 1/4, 1/2, 1, 2} -- every product and every partial sum
is a multiple of 1/4 below 2^22, so a float32 sum is the same in any order, with or without fma, and equals float64 bit for bit: one
dropped, doubled or misplaced entry changes bits.  general_data: normal rows and arbitrary weights, held to the worst-case bound
of a length-L fma chain, bound()."""
import numpy as np

CLASSES = (1, 2, 3, 4, 5, 7, 8, 9)     # list lengths placed on purpose (0 besides): the 4-way unrolled walk and its tail
EXACT_W = np.array([1.0, 0.5, 0.25, 2.0], np.float32)
U = 2.0 ** -24                         # unit roundoff of float32


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    return f32(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the operation
def scatter_f64(idx, rows, w, div, nsrc):
    """idx (b, nent) ints in [0, nsrc); rows (b, nent // div, c); w (b, nent) or None (= 1) -> out (b, nsrc, c) float64, sum_abs
    (the same sum over |w * rows|) and L (b, nsrc): entries per source"""
    idx = np.asarray(idx)
    b, nent = idx.shape
    rows = np.asarray(rows, np.float64)
    c = rows.shape[2]
    assert rows.shape[:2] == (b, nent // div) and nent % div == 0
    out, sum_abs = np.zeros((b, nsrc, c)), np.zeros((b, nsrc, c))
    L = np.zeros((b, nsrc), np.int64)
    src_row = np.arange(nent) // div
    for bi in range(b):
        t = rows[bi][src_row]
        if w is not None:
            t = t * np.asarray(w[bi], np.float64).reshape(nent, 1)
        np.add.at(out[bi], idx[bi], t)
        np.add.at(sum_abs[bi], idx[bi], np.abs(t))
        L[bi] = np.bincount(idx[bi], minlength=nsrc)
    return out, sum_abs, L


def weights_f32(dist):
    """weight_kind 2 as the kernels spell it, every operation rounded to float32: r_j = 1 / max(d_j, 1e-10),
    norm = (r1 + r2) + r3, w_j = r_j / norm.  dist (..., 3) squared distances -> (..., 3) float32"""
    d = np.maximum(f32(dist), np.float32(1e-10))
    with np.errstate(divide="ignore"):
        r = np.float32(1.0) / d
    norm = (r[..., 0] + r[..., 1]) + r[..., 2]
    w = r / norm[..., None]
    assert w.dtype == np.float32
    return w


def entry_weights(b, nent, kind, wdata):
    """the float32 weight of every entry (b, nent) for a build of `kind` with operand `wdata` (None / weights / distances)"""
    if kind == 0:
        return np.ones((b, nent), np.float32)
    if kind == 1:
        return f32(wdata).reshape(b, nent)
    return weights_f32(f32(wdata).reshape(b, nent // 3, 3)).reshape(b, nent)


def bound(sum_abs, L):
    """|float32 result - float64 result| of a length-L chain acc = fma(row, w, acc) in ANY order: each of the L roundings is at most
    2^-24 of a partial sum, itself at most sum_abs (1 + L 2^-24); + 1 for those second-order terms (L < 2^20), + 1 for nothing:
    (L + 2) 2^-24 sum_abs.  An empty list gives exactly 0."""
    return (np.asarray(L, np.float64)[..., None] + 2.0) * U * sum_abs


def ordered_sums_f32(idx, rows, w, div, nsrc, rs, fma):
    """what a kernel may compute: per source a sequential float32 sum over its list in a random order.  fma False: the product is
    rounded to float32, then the sum; True: the product is exact (float64 holds 24 x 24 bits) and the sum is rounded once (to 53
    bits on the way, which is below anything asserted here)"""
    idx = np.asarray(idx)
    b, nent = idx.shape
    rows = f32(rows)
    c = rows.shape[2]
    n = b * nent
    gsrc = (idx.astype(np.int64) + np.arange(b)[:, None] * nsrc).reshape(n)      # clouds side by side: b * nsrc sources
    grow = (np.arange(nent)[None, :] // div + np.arange(b)[:, None] * (nent // div)).reshape(n)
    order = np.lexsort((rs.rand(n), gsrc))
    src = gsrc[order]
    cnt = np.bincount(src, minlength=b * nsrc)
    start = np.cumsum(cnt) - cnt
    pos = np.arange(n) - start[src]
    r = rows.reshape(-1, c)[grow[order]]
    wt = np.ones((n, 1), np.float32) if w is None else f32(w).reshape(n)[order].reshape(n, 1)
    prod = r.astype(np.float64) * wt.astype(np.float64) if fma else r * wt
    out = np.zeros((b * nsrc, c), np.float32)
    short = 16
    by_pos = np.argsort(pos, kind="stable")
    ends = np.cumsum(np.bincount(pos, minlength=1))
    lo = 0
    for hi in ends[:short]:                   # step k: the k-th entry of every list that has one (distinct sources)
        sel = by_pos[lo:hi]
        if fma:
            out[src[sel]] = (out[src[sel]].astype(np.float64) + prod[sel]).astype(np.float32)
        else:
            out[src[sel]] = out[src[sel]] + prod[sel]
        lo = hi
    for s in np.flatnonzero(cnt > short):     # the few long lists one by one, from where the steps above left them
        seg = prod[start[s] + short:start[s] + cnt[s]]
        if fma:
            acc = out[s]
            for t in seg:
                acc = (acc.astype(np.float64) + t).astype(np.float32)
            out[s] = acc
        else:                                 # accumulate is sequential by definition: every prefix is an output
            out[s] = np.add.accumulate(np.concatenate([out[s][None], seg]), axis=0, dtype=np.float32)[-1]
    return out.reshape(b, nsrc, c)


def scatter_naive(idx, rows, w, div, nsrc):
    """the triple loop scatter_f64 is checked against"""
    b, nent = np.shape(idx)
    c = np.shape(rows)[2]
    out, sa = np.zeros((b, nsrc, c)), np.zeros((b, nsrc, c))
    L = np.zeros((b, nsrc), np.int64)
    for bi in range(b):
        for e in range(nent):
            s = int(idx[bi][e])
            L[bi, s] += 1
            for ch in range(c):
                t = float(rows[bi][e // div][ch]) * (1.0 if w is None else float(w[bi][e]))
                out[bi, s, ch] += t
                sa[bi, s, ch] += abs(t)
    return out, sa, L


# ------------------------------------------------------------------------------------------------------------------ the plan
def plan_words(b, nent, nsrc):
    return 2 * b * nsrc + 2 * b * nent


def decode_plan(raw_bytes, b, nent, nsrc):
    """the layout above pn2_scatter_plan_bytes: int32 cursor[b][nsrc] (after a build: the list lengths) | offset[b][nsrc] |
    entry row[b][nent] | float32 entry weight[b][nent] -> cnt, off, eq, ew"""
    a = np.frombuffer(bytes(raw_bytes) if not isinstance(raw_bytes, np.ndarray) else raw_bytes.tobytes(), np.int32)
    assert a.size == plan_words(b, nent, nsrc), "a plan of %d words, expected %d" % (a.size, plan_words(b, nent, nsrc))
    p = b * nsrc
    return (a[:p].reshape(b, nsrc).copy(), a[p:2 * p].reshape(b, nsrc).copy(), a[2 * p:2 * p + b * nent].reshape(b, nent).copy(),
            a[2 * p + b * nent:].view(np.float32).reshape(b, nent).copy())


def encode_plan(cnt, off, eq, ew):
    return np.concatenate([np.asarray(cnt, np.int32).ravel(), np.asarray(off, np.int32).ravel(), np.asarray(eq, np.int32).ravel(),
                           f32(ew).ravel().view(np.int32)]).tobytes()


def build_plan_host(idx, w32, div, nsrc, rs=None):
    """a valid plan from the host (lists in entry order, or shuffled inside each list with rs) -> cnt, off, eq, ew"""
    idx = np.asarray(idx)
    b, nent = idx.shape
    cnt = np.stack([np.bincount(idx[bi], minlength=nsrc) for bi in range(b)]).astype(np.int32)
    off = (np.cumsum(cnt, axis=1) - cnt).astype(np.int32)
    eq, ew = np.zeros((b, nent), np.int32), np.zeros((b, nent), np.float32)
    for bi in range(b):
        order = np.lexsort((np.arange(nent) if rs is None else rs.rand(nent), idx[bi]))
        eq[bi], ew[bi] = order // div, f32(w32[bi])[order]
    return cnt, off, eq, ew


def check_plan(cnt, off, eq, ew, idx, w32, div, nsrc):
    """AssertionError unless, per cloud: cnt = bincount(idx), off = its exclusive scan, and for every source the multiset of
    (row, weight bits) in its list is {(e // div, bits of w32[e]) : idx[e] == source}.  The order inside a list is free."""
    idx = np.asarray(idx)
    b, nent = idx.shape
    assert cnt.shape == off.shape == (b, nsrc) and eq.shape == ew.shape == (b, nent)
    for bi in range(b):
        n = np.bincount(idx[bi], minlength=nsrc)
        assert np.array_equal(cnt[bi], n), "cloud %d: list lengths differ from bincount(idx) at sources %s" % (
            bi, np.flatnonzero(cnt[bi] != n)[:8])
        scan = np.cumsum(n) - n
        assert np.array_equal(off[bi], scan), "cloud %d: offsets are not the exclusive scan, first at source %d" % (
            bi, np.flatnonzero(off[bi] != scan)[0])
        owner = np.repeat(np.arange(nsrc), n)                         # source of every list position
        gb, wb = bits(ew[bi]).astype(np.int64), bits(w32[bi]).astype(np.int64)
        got = np.lexsort((gb, eq[bi], owner))
        want = np.lexsort((wb, np.arange(nent) // div, idx[bi]))
        same = (owner[got] == idx[bi][want]) & (eq[bi][got] == (np.arange(nent) // div)[want]) & (gb[got] == wb[want])
        assert same.all(), "cloud %d: %d list entries are not the (row, weight) of an index entry of their source, first in source %d" % (
            bi, int((~same).sum()), int(owner[got][np.flatnonzero(~same)[0]]))


# --------------------------------------------------------------------------------------------------------------- index tables
def make_idx(b, nsrc, nrows, div, seed, phase=0):
    """(b, nrows * div) int32 in [0, nsrc), a different table per cloud.  As far as nent = nrows * div entries and nsrc sources
    allow, per cloud: sources of list length 1, 2, 3, 4, 5, 7, 8, 9 (CLASSES) at random places and sources of length 0; one hot
    source with half of what is left; source 0 empty in the clouds with (cloud + phase) even, source nsrc - 1 empty in those with
    (cloud + phase) // 2 even, both non-empty otherwise (nsrc >= 3, enough entries); with div == 3 the hot source's entries fill
    whole input rows (all three indices equal).  The rest is spread at random."""
    rs = np.random.RandomState(seed)
    nent = nrows * div
    out = np.zeros((b, nent), np.int32)
    for bi in range(b):
        length = np.zeros(nsrc, np.int64)
        left = nent
        first_empty, last_empty = (bi + phase) % 2 == 0, ((bi + phase) // 2) % 2 == 0
        closed = set()
        if nsrc >= 3:
            closed = ({0} if first_empty else set()) | ({nsrc - 1} if last_empty else set())
        free = [s for s in rs.permutation(nsrc) if s not in closed and s not in (0, nsrc - 1)]
        ends = [s for s in (0, nsrc - 1) if s not in closed][:nsrc]
        free = list(dict.fromkeys(ends + free))            # the open ends take the first classes
        for k in np.roll(CLASSES, -bi):                    # one source stays free for the hot one
            if len(free) > 1 and left >= k:
                length[free.pop(0)], left = k, left - k
        hot = free.pop(0)
        share = (left + 1) // 2 if free else left
        if div == 3:
            share = min(left, -(-share // 3) * 3) if left >= 3 else share
        length[hot] += share
        left -= share
        if left:
            if len(free) > 1:
                free = free[:max(1, len(free) // 2)]       # half of the remaining sources stay empty
            length += np.bincount(rs.choice(free, left), minlength=nsrc)
        assert length.sum() == nent and not any(length[s] for s in closed)
        ent = np.repeat(np.arange(nsrc), length)
        rest = ent[ent != hot] if length[hot] < nent else ent[:0]
        nhot = nent - rest.size
        rest = rs.permutation(rest)
        if div == 3:
            whole = nhot // 3 * 3
            table = np.concatenate([np.full(whole, hot), rs.permutation(np.concatenate([np.full(nhot - whole, hot), rest]))])
            table = table.reshape(nrows, 3)[rs.permutation(nrows)].reshape(-1)
        else:
            table = rs.permutation(np.concatenate([np.full(nhot, hot), rest]))
        out[bi] = table
    return out


def idx_facts(idx, nsrc, div):
    """what make_idx is asked for, as found in a table: the set of list lengths <= 9, (first source empty, last source empty) per
    cloud, the largest share of one source, rows with all `div` indices equal"""
    idx = np.asarray(idx)
    lens, ends, share, rows_equal = set(), [], 0.0, 0
    for t in idx:
        n = np.bincount(t, minlength=nsrc)
        lens |= set(int(v) for v in n if v <= 9)
        ends.append((n[0] == 0, n[-1] == 0))
        share = max(share, n.max() / float(t.size))
        r = t.reshape(-1, div)
        rows_equal += int((r == r[:, :1]).all(axis=1).sum()) if div > 1 else 0
    return lens, ends, share, rows_equal


# ----------------------------------------------------------------------------------------------------------------------- data
def exact_data(idx, div, c, kind, seed):
    """rows (b, nent // div, c) of integers in [-8, 8] and the build's weight operand: None (kind 0), weights from {1, 1/2, 1/4, 2}
    (kind 1), or squared distances (kind 2) whose float32 weights are exact: (d, d, d/2) -> (1/4, 1/4, 1/2), (d, d, inf) ->
    (1/2, 1/2, 0), (d, inf, inf) -> (1, 0, 0) in any of the three positions, d a power of two"""
    b, nent = np.shape(idx)
    rs = np.random.RandomState(seed)
    rows = rs.randint(-8, 9, (b, nent // div, c)).astype(np.float32)
    if kind == 0:
        return rows, None
    if kind == 1:
        return rows, EXACT_W[rs.randint(0, 4, (b, nent))]
    assert div == 3
    n = nent // 3
    d = (2.0 ** rs.randint(-6, 7, (b, n, 1))).astype(np.float32)
    pat = np.array([[1.0, 1.0, 0.5], [1.0, 1.0, np.inf], [1.0, np.inf, np.inf]], np.float32)[rs.randint(0, 3, (b, n))]
    dist = d * np.take_along_axis(pat, np.argsort(rs.rand(b, n, 3), axis=2), axis=2)
    return rows, f32(dist)


def general_data(idx, div, c, kind, seed):
    """normal rows; kind 1: positive weights normalised per row group; kind 2: positive distances over six decades, every fifth row
    with one zero and every seventh with two (the 1e-10 clamp)"""
    b, nent = np.shape(idx)
    rs = np.random.RandomState(seed)
    rows = rs.randn(b, nent // div, c).astype(np.float32)
    if kind == 0:
        return rows, None
    if kind == 1:
        w = rs.rand(b, nent // div, div) + 0.01
        return rows, f32(w / w.sum(2, keepdims=True)).reshape(b, nent)
    dist = (10.0 ** rs.uniform(-4, 2, (b, nent // 3, 3))).astype(np.float32)
    dist[:, ::5, 1] = 0.0
    dist[:, ::7, :2] = 0.0
    return rows, dist


def is_exact(rows, w32, idx, div, nsrc):
    """the premise of the exactness claim, checked on the data itself: every product is a multiple of 1/4 and every sum of |products|
    stays below 2^22 (so 4 x any partial sum is an integer below 2^24)"""
    _, sa, _ = scatter_f64(idx, rows, w32, div, nsrc)
    t = np.asarray(rows, np.float64)[:, np.arange(np.shape(idx)[1]) // div] * np.asarray(w32, np.float64)[..., None]
    return bool((t * 4 == np.round(t * 4)).all() and sa.max() < 2.0 ** 22)


# --------------------------------------------------------------------------------------------------------------------- shapes
APPLY_C = (4, 8, 12, 20, 36, 132, 260, 512, 516, 1020, 1024)
MODES = ((1, 0), (3, 1), (3, 2))            # (div, weight_kind)


def spb(c):
    return 256 // (c // 4)                  # sources per block of the gather


def apply_nsrc(c):
    s = spb(c)
    return sorted(set(v for v in (1, s - 1, s, s + 1, 3 * s + 1) if v > 0))


def apply_rows(nsrc, div):
    """input rows of an apply case: room for every class, a hot source and a spread over the other sources"""
    return (96 + nsrc) // div + 8


def apply_cases():
    """(c, nsrc, b, div, kind) of the column sweep"""
    return [(c, nsrc, b, div, kind) for c in APPLY_C for nsrc in apply_nsrc(c) for b in (1, 3) for div, kind in MODES]


def case_seed(*v):
    s = 17
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return s


def apply_case(c, nsrc, b, div, kind, exact=True):
    """idx, rows, weight operand, float32 entry weights of one case"""
    seed = case_seed(c, nsrc, b, div, kind)
    idx = make_idx(b, nsrc, apply_rows(nsrc, div), div, seed, phase=c // 4 + nsrc)
    rows, wdata = (exact_data if exact else general_data)(idx, div, c, kind, seed + 1)
    return idx, rows, wdata, entry_weights(b, idx.shape[1], kind, wdata)


BUILD_NSRC = (1, 2, 255, 256, 257, 511, 513)
BUILD_ROWS = (1, 255, 256, 257)             # nent = rows * div


def build_cases():
    """(b, nsrc, nrows, div, kind) of the single build; the last three: grid-stride loops (block cap ceil(2048 / 64) = 32 of 256)"""
    cases = [(2, nsrc, rows, div, kind) for nsrc in BUILD_NSRC for rows in BUILD_ROWS for div, kind in MODES]
    return cases + [(64, 257, 8192 + 257, 1, 0), (64, 257, (8192 + 257 + 2) // 3, 3, 1), (64, 257, (8192 + 257 + 2) // 3, 3, 2)]


def build_case(b, nsrc, nrows, div, kind, exact=True, c=4):
    seed = case_seed(b, nsrc, nrows, div, kind, 5)
    idx = make_idx(b, nsrc, nrows, div, seed, phase=nsrc + nrows)
    rows, wdata = (exact_data if exact else general_data)(idx, div, c, kind, seed + 1)
    return idx, rows, wdata, entry_weights(b, idx.shape[1], kind, wdata)


# source counts of the batches built at once: mixed under one max_src; 16384 is the last count the one-launch LDS path takes
MULTI_BATCHES = {
    "lds8": (1, 63, 64, 65, 1023, 1024, 1025, 2049),
    "lds8_max": (65, 16384, 1, 1025, 2049, 64, 1023, 63),
    "lds1_max": (16384,),
    "lds1_one": (1,),
    "lds1_1025": (1025,),
    "global8": (65, 16385, 1, 1025, 2049, 64, 1023, 63),
}
# clouds per batch: three where the plans are small (an odd count leaves plans that end 8 bytes off a 16-byte boundary)
MULTI_B = {"lds8": 3, "lds8_max": 2, "lds1_max": 2, "lds1_one": 3, "lds1_1025": 3, "global8": 2}


def multi_rows(nsrc, div):
    """input rows of a plan of a multi batch: about one entry per source up to a few thousand entries"""
    return (min(max(nsrc, 24) + 75, 4200)) // div + 1


def multi_specs(name):
    """[(nsrc, nrows, div, kind)] of a batch: kinds 0 / 1 / 2 in turn"""
    return [(nsrc, multi_rows(nsrc, MODES[i % 3][0]),) + MODES[i % 3] for i, nsrc in enumerate(MULTI_BATCHES[name])]


def multi_case(name, i, c=4):
    nsrc, nrows, div, kind = multi_specs(name)[i]
    seed = case_seed(nsrc, nrows, div, kind, i, 9)
    b = MULTI_B[name]
    idx = make_idx(b, nsrc, nrows, div, seed, phase=i)
    rows, wdata = exact_data(idx, div, c, kind, seed + 1)
    return idx, rows, wdata, entry_weights(b, idx.shape[1], kind, wdata)


# general data: one shape per c class of the gather (cv = c / 4 divides 256 or leaves idle threads, one source per block), the hot
# source in each, kind 2 with clamped distances
GENERAL_CASES = [(4, 257, 3, 1, 0), (12, 86, 3, 3, 1), (36, 29, 1, 3, 2), (132, 8, 3, 3, 2), (260, 4, 3, 1, 0), (512, 7, 1, 3, 1),
                 (516, 2, 3, 3, 2), (1020, 4, 1, 3, 1), (1024, 4, 3, 3, 2)]
