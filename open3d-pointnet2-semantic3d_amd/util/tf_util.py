"""Layer helpers with the reference's names and maths, torch/HIP underneath.

Mirrors the subset of util/tf_util.py the SA/FP stack uses: conv2d (1x1 only,
:128-204), conv1d (kernel 1 only, :54-125), batch norm (:555-581, epsilon 1e-3,
center+scale, moving averages updated in place), dropout (:646-665), xavier
weights / zero biases (:30-51,109-111).  TF's implicit variable scopes become an
explicit VariableStore (name -> tensor) so the reference's functional layer API
(`scope=` strings) can be kept.

Two execution paths per layer:
  * is_training=False -> the BatchNorm is folded into (W, b) and the layer runs on
    the hand-written fp32-MFMA kernels of libpn2_hip.so (pn2_linear / fused SA);
  * is_training=True  -> differentiable torch ops (batch statistics cannot be
    fused through; the index/gather ops around it are still the HIP kernels).
"""
import contextlib
import math
from collections import OrderedDict, namedtuple

import weakref

import torch
import torch.nn.functional as F

from .._lib import BN_WS_FOLDED, BN_WS_SUMMED, BN_WS_UNCLEARED, BN_WS_ZEROED
from .._lib import int_array, launch, layer_arrays, lib, nbytes, ptr, ptr_table, require_cuda, rows_in_place, u64_array

BN_EPSILON = 1e-3  # tf.contrib.layers.batch_norm default (tf_util.py:571-581)


class VariableStore:
    """name -> tensor registry standing in for TF's variable scopes."""

    def __init__(self, device="cuda", seed=0):
        self.device = torch.device(device)
        self.params = OrderedDict()   # trainable
        self.buffers = OrderedDict()  # moving averages
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(seed)
        self._seed = int(seed)
        self._dropout = {}
        self._folded = {}
        self.zero_arena = None  # ZeroArena of the training step (set by train.Trainer), None = every call zero-fills its own scratch
        # direct gradients (train.Trainer): parameter storage address -> (flat gradient buffer, offset, numel).  While
        # `grad_direct` is set -- inside a trainer's forward/backward, which zero-fills the flat buffer first -- the weight-gradient
        # and batch-norm kernels write each parameter's gradient straight into its slice (grad_view): no per-step pack copy
        self.grad_map = {}
        self.grad_direct = False
        self.train_epoch = 0  # bumped by every training-mode layer call: the HIP BN kernel updates the moving averages
                              # through raw pointers (no autograd version bump), so folded inference weights key on it too

    def grad_view(self, t):
        """a FRESH view, shaped like t, of the flat-gradient slice of the parameter whose storage t shares, or None (no trainer
        bound / outside its backward).  Fresh: autograd keeps a returned gradient without a copy only when nothing else holds it."""
        if not self.grad_direct:
            return None
        ent = self.grad_map.get(t.data_ptr())
        if ent is None or ent[2] != t.numel():
            return None
        flat, off, n = ent
        return flat[off:off + n].view(t.shape)

    def dropout_state(self, key, salt):
        """device int64[2] = {seed ^ salt, step} of one dropout call site; `set_step` advances every site."""
        t = self._dropout.get(key)
        if t is None:
            t = torch.tensor([(self._seed * 0x9E3779B1 + 12345) ^ int(salt), 0], dtype=torch.int64, device=self.device)
            self._dropout[key] = t
        return t

    def step_fills(self, step):
        """[(tensor, value)] that set_step would write: for a launch that stores them itself (tf_util.multi_copy_(fills=))"""
        return [(t[1:2], int(step)) for t in self._dropout.values()]

    def set_step(self, step):
        # a fill KERNEL on the current stream.  (`t[1] = int(step)` is a host-to-device copy of a pageable scalar: it blocks
        # the host until everything queued before it has run -- measured 4.2 ms per training step, tools/train_host_probe.py)
        for t in self._dropout.values():
            t[1:2].fill_(int(step))

    def get_variable(self, name, shape, init):
        if name not in self.params:
            self.params[name] = torch.nn.Parameter(init(shape).to(self.device))
        p = self.params[name]
        if tuple(p.shape) != tuple(shape):
            raise ValueError("variable %s exists with shape %s, requested %s" % (name, tuple(p.shape), tuple(shape)))
        return p

    def get_buffer(self, name, shape, value):
        if name not in self.buffers:
            self.buffers[name] = torch.full(shape, float(value), dtype=torch.float32, device=self.device)
        return self.buffers[name]

    def xavier(self, shape):
        # tf.contrib.layers.xavier_initializer(uniform=True): limit = sqrt(6 / (fan_in + fan_out))
        receptive = 1
        for d in shape[:-2]:
            receptive *= d
        fan_in, fan_out = shape[-2] * receptive, shape[-1] * receptive
        limit = math.sqrt(6.0 / (fan_in + fan_out))
        return (torch.rand(shape, generator=self._gen, dtype=torch.float32) * 2 - 1) * limit

    def parameters(self):
        return list(self.params.values())

    def num_parameters(self):
        return sum(p.numel() for p in self.params.values())

    def state_dict(self):
        d = OrderedDict((k, v.detach().clone()) for k, v in self.params.items())
        d.update((k, v.clone()) for k, v in self.buffers.items())
        return d

    def load_state_dict(self, state):
        with torch.no_grad():
            for k, v in state.items():
                tgt = self.params.get(k, self.buffers.get(k))
                if tgt is None:
                    raise KeyError(k)
                tgt.copy_(v.to(self.device))

    # folded inference weights, cached on the version counters of their sources
    def folded(self, key, sources, make):
        stamp = (self.train_epoch,) + tuple((id(t), t._version) for t in sources)
        hit = self._folded.get(key)
        if hit is None or hit[0] != stamp:
            with torch.no_grad():
                hit = (stamp, make())
            self._folded[key] = hit
        return hit[1]


class ZeroArena:
    """Per-step scratch that must START OUT ZERO (batch-norm accumulators, weight-gradient tiles that are added to with
    atomics).  `reset()` zero-fills the whole arena with ONE launch and rewinds it; `take(nbytes)` hands out consecutive
    256-byte aligned slices.  Replaces one memset per layer call (~110 per training step).  The first step runs
    without an arena and only measures (`needed`); the trainer then allocates it."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = None
        self.off = 0
        self.needed = 0
        self._count = 0

    def allocate(self):
        self.buf = torch.zeros(max(256, self.needed + 256), dtype=torch.uint8, device=self.device)
        self.off = 0

    def reset(self):
        self._count = 0
        if self.buf is not None:
            self.buf.zero_()
            self.off = 0

    def take(self, nbytes):
        """-> a zero-filled uint8 view of nbytes, or None when the arena is not allocated yet / exhausted (the caller then
        uses the self-zeroing entry point)."""
        nbytes = (int(nbytes) + 255) & ~255
        self._count += nbytes
        if self._count > self.needed:
            self.needed = self._count
        if self.buf is None or self.off + nbytes > self.buf.numel():
            return None
        v = self.buf[self.off:self.off + nbytes]
        self.off += nbytes
        return v


_default_store = None
_scope_stack = []


def get_default_store():
    global _default_store
    if _default_store is None:
        _default_store = VariableStore()
    return _default_store


def set_default_store(store):
    global _default_store
    _default_store = store
    return store


@contextlib.contextmanager
def variable_scope(name):
    _scope_stack.append(name)
    try:
        yield "/".join(_scope_stack)
    finally:
        _scope_stack.pop()


def _full_name(leaf):
    return "/".join(_scope_stack + [leaf])


def _dense_variables(cin, cout, bn, kernel_shape):
    st = get_default_store()
    w = st.get_variable(_full_name("weights"), kernel_shape, st.xavier)
    b = st.get_variable(_full_name("biases"), (cout,), lambda s: torch.zeros(s))
    if not bn:
        return st, w, b, None
    with variable_scope("bn"):
        beta = st.get_variable(_full_name("beta"), (cout,), lambda s: torch.zeros(s))
        gamma = st.get_variable(_full_name("gamma"), (cout,), lambda s: torch.ones(s))
        mean = st.get_buffer(_full_name("moving_mean"), (cout,), 0.0)
        var = st.get_buffer(_full_name("moving_variance"), (cout,), 1.0)
    return st, w, b, (beta, gamma, mean, var)


def folded_dense(cin, cout, bn, kernel_shape, pad_to=None, pad_in=None, rotate_rows=0):
    """(W', b') with the inference BatchNorm folded in:
    y = (x@W + b - mean)/sqrt(var+eps)*gamma + beta = x@(W*s) + ((b-mean)*s + beta).
    rotate_rows = r moves the LAST r input rows of W' to the front (a kernel that feeds [xyz | features] to a
    layer whose variables were created for [features | xyz], pointnet_util.py:259)."""
    st, w, b, bnv = _dense_variables(cin, cout, bn, kernel_shape)
    key = (_full_name("folded"), pad_to, pad_in, rotate_rows)

    def make():
        w2 = w.detach().reshape(cin, cout)
        b2 = b.detach()
        if bnv is not None:
            beta, gamma, mean, var = bnv
            s = gamma.detach() / torch.sqrt(var + BN_EPSILON)
            w2 = w2 * s
            b2 = (b2 - mean) * s + beta.detach()
        if pad_to is not None and cout % pad_to != 0:
            padc = pad_to - cout % pad_to
            w2 = F.pad(w2, (0, padc))
            b2 = F.pad(b2, (0, padc))
        if rotate_rows:
            w2 = torch.cat([w2[cin - rotate_rows:], w2[:cin - rotate_rows]], dim=0)
        if pad_in is not None and pad_in > cin:  # zero rows for zero-padded input columns
            w2 = F.pad(w2, (0, 0, 0, pad_in - cin))
        return w2.contiguous(), b2.contiguous()

    srcs = [w, b] + (list(bnv) if bnv is not None else [])
    return st.folded(key, srcs, make)


def hip_linear(x2d, w, b, relu=True, pool=0):
    """y = relu?(x2d @ w + b), optional max over groups of `pool` consecutive rows.
    Thin wrapper over pn2_linear (fp32 MFMA)."""
    require_cuda(x2d, w, b)  # b may be None (no bias)
    rows, cin = x2d.shape
    cout = w.shape[1]
    x2d = x2d.contiguous()
    orows = rows // pool if pool and pool > 1 else rows
    y = torch.empty((orows, cout), dtype=torch.float32, device=x2d.device)
    launch("pn2_linear", x2d, rows, cin, cout, ptr(x2d), ptr(w), ptr(b), int(bool(relu)), int(pool or 0), ptr(y))
    return y


def hip_linear_pool_packed(x2d, idx, w, b):
    """relu(max over each group of 32 rows of x2d @ w + b) on the live rows of the ball query `idx` (b, m, 32) only
    (pn2_linear_pool_packed): x2d's rows behind a padded index entry must be copies of the group's first row, which holds for the
    output of the fused gather chain on `idx`.  Same bits as hip_linear(..., relu=True, pool=32).
    -> (b * m, cout), or None when the library refuses the configuration (caller falls back to hip_linear)."""
    require_cuda(x2d, idx, w, b)
    groups, nsample = idx.shape[0] * idx.shape[1], idx.shape[2]
    cin, cout = w.shape
    x2d, idx = x2d.contiguous(), idx.contiguous()
    y = torch.empty((groups, cout), dtype=torch.float32, device=x2d.device)
    ok = launch("pn2_linear_pool_packed", x2d, groups, nsample, cin, cout, ptr(x2d), ptr(idx), ptr(w), ptr(b), 1, ptr(y),
                may_refuse=True)
    return y if ok else None


_SAME = object()


def _launch_stack(name, where, lead, ws, bs, trail, oshape, w0=_SAME, after=()):
    """One launch of a fused-MLP entry point: name(*lead, nlayers, widths[], w[], bias[], *trail, y, *after, stream) with y a new
    float32 tensor of `oshape` on the device of `where`.  lead / trail / after hold the scalars and the tensors (None -> NULL)
    in the prototype's order; the tensors are dense already and are held until the call has returned.  ws, bs: the layers'
    (cin_i, cout_i) weights and biases; w0 replaces the pointer of the first layer's weight where the entry point reads other
    rows than ws[0]'s (a padded or split first layer; None -> NULL).
    -> y, or None when the library reports the configuration as unsupported.  Every other failure raises Pn2Error."""
    L, widths, wptrs, bptrs = layer_arrays(ws, bs)
    if w0 is not _SAME:
        wptrs = ptr_table([w0] + list(ws[1:]))
    y = torch.empty(oshape, dtype=torch.float32, device=where.device)
    dev = lambda args: [ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]  # noqa: E731
    ok = launch(name, where, *dev(lead), L, widths, wptrs, bptrs, *dev(trail), ptr(y), *dev(after), may_refuse=True)
    return y if ok else None


def pad_first_layer_rows(w0, cin):
    """W0 zero-padded to cin rounded up to a multiple of 8 rows: the wide kernels read W0 in groups of 8 rows"""
    need = -(-cin // 8) * 8
    return w0 if w0.shape[0] >= need else F.pad(w0, (0, 0, 0, need - w0.shape[0])).contiguous()


def hip_mlp_chain(x2d, ws, bs, pool=0):
    """relu(relu(x @ W0 + b0) @ W1 + b1) with LDS-resident weights (pn2_mlp_chain).  Returns None
    when the library reports the configuration as unsupported (caller falls back to hip_linear)."""
    require_cuda(x2d)
    rows, cin = x2d.shape
    return _launch_stack("pn2_mlp_chain", x2d, (rows, cin, x2d.contiguous()), ws, bs, (int(pool),),
                         (rows // pool if pool else rows, ws[-1].shape[1]))


def multi_copy_(dsts, srcs, fills=()):
    """dsts[i].copy_(srcs[i]) for lists of contiguous device tensors of any dtypes in ONE launch (pn2_multi_copy);
    torch._foreach_copy_ issues one memcpy per tensor when the dtypes are mixed.  fills = [(one-element float32 / int64 tensor,
    python value), ...] (<= 4): scalars stored by the same launch, their values travelling in the launch arguments
    (pn2_multi_copy_fill) -- a training step's lr_t and dropout step ride with its input copy."""
    import struct
    n = len(dsts)
    if n != len(srcs):
        raise ValueError("multi_copy_: list lengths differ")
    for d, s in zip(dsts, srcs):
        if nbytes(d) != nbytes(s) or not d.is_contiguous() or not s.is_contiguous():
            raise ValueError("multi_copy_: contiguous tensors of equal byte size expected")
    from ..tf_ops.tf_sampling import drop_fps_tag
    for d in dsts:
        drop_fps_tag(d)  # a write through the raw pointer: no version counter moves, so the tie-record tag must not survive it
    fills = list(fills)
    if len(fills) > 4:
        raise ValueError("multi_copy_: at most 4 scalar fills")
    for i0 in range(0, n, 48):
        dd, ss = dsts[i0:i0 + 48], srcs[i0:i0 + 48]
        k = len(dd)
        sp, dp = ptr_table(ss), ptr_table(dd)
        nb = u64_array([nbytes(t) for t in dd])
        if fills and i0 == 0:
            vals, sizes = [], []
            for t, v in fills:
                if t.numel() != 1 or t.dtype not in (torch.float32, torch.int64):
                    raise ValueError("multi_copy_: a fill target is one float32 or int64 element")
                if t.dtype == torch.float32:
                    vals.append(struct.unpack("<I", struct.pack("<f", float(v)))[0])  # the float's bits, widened
                    sizes.append(4)
                else:
                    vals.append(int(v) & 0xFFFFFFFFFFFFFFFF)
                    sizes.append(8)
            launch("pn2_multi_copy_fill", dd[0], k, sp, dp, nb, len(fills), ptr_table([t for t, _ in fills]), u64_array(vals),
                   int_array(sizes))
        else:
            launch("pn2_multi_copy", dd[0], k, sp, dp, nb)


def hip_mlp_wide(x2d, ws, bs, relu_last=True, pool=0):
    """up to three dense layers of width 128 / 256 / 512 in ONE launch (pn2_mlp_wide: a workgroup carries a 32-row tile
    through all layers); pool = 32 adds the max over each group of 32 rows.  None when the library reports the
    configuration as unsupported (caller falls back to hip_linear per layer)."""
    require_cuda(x2d)
    rows, cin = x2d.shape
    return _launch_stack("pn2_mlp_wide", x2d, (rows, cin, cin, x2d.contiguous()), ws, bs, (int(bool(relu_last)), int(pool)),
                         (rows // pool if pool else rows, ws[-1].shape[1]), w0=pad_first_layer_rows(ws[0], cin))


def _fp_shapes(dist, points1, points2):
    b, n, _ = dist.shape
    return b, n, points2.shape[1], (0 if points1 is None else points1.shape[2]), points2.shape[2]


def hip_fp_mlp_wide(dist, idx, points1, points2, ws, bs):
    """[three_interpolate(points2) | points1] -> up to three wide dense layers in ONE launch (pn2_fp_mlp_wide);
    -> (b*n, w_last) or None when the library reports the configuration as unsupported."""
    require_cuda(dist, idx, points1, points2)
    b, n, m, c1, c2 = _fp_shapes(dist, points1, points2)
    p1 = None if points1 is None else points1.contiguous()
    return _launch_stack("pn2_fp_mlp_wide", dist, (b, n, m, c1, c2, dist.contiguous(), idx.contiguous(), p1, points2.contiguous()),
                         ws, bs, (), (b * n, ws[-1].shape[1]), w0=pad_first_layer_rows(ws[0], c1 + c2))


def sa_wide_first_layer(w0):
    """W0 (3 + c, cout) in the reference's [xyz | features] row order (pointnet_util.py:52-54) -> the row order
    pn2_sa_mlp_wide reads: [features | xyz | zero rows up to a multiple of 8]"""
    w = torch.cat([w0[3:], w0[:3]], dim=0)
    return pad_first_layer_rows(w, w.shape[0]).contiguous()


def _sa_out_shape(idx, wl, pool):
    b, m, ns = idx.shape
    return (b, m, wl) if pool else (b, m, ns, wl)


def hip_sa_mlp_wide(xyz, new_xyz, points, idx, ws, bs, pool=True):
    """SA front end (gather, centre, concat) + up to three wide dense layers + max over the 32 neighbours in ONE launch
    (pn2_sa_mlp_wide).  ws[0] in the kernel's row order (sa_wide_first_layer / folded_dense(rotate_rows, pad_in)).
    -> (b, m, w_last) (pool) or (b, m, 32, w_last); None when unsupported."""
    require_cuda(xyz, new_xyz, points, idx)
    b, n, _ = xyz.shape
    m, ns = idx.shape[1], idx.shape[2]
    lead = (b, n, m, ns, points.shape[2], xyz.contiguous(), new_xyz.contiguous(), points.contiguous(), idx.contiguous())
    return _launch_stack("pn2_sa_mlp_wide", xyz, lead, ws, bs, (int(bool(pool)),), _sa_out_shape(idx, ws[-1].shape[1], pool))


def hip_fp_mlp_wide_pre(dist, idx, points1, points2, ws, bs):
    """pn2_fp_mlp_wide with the first layer hoisted by linearity (see hip_fp_mlp_fused_pre): z = points2 @ W0[:c2] on the
    known points; the kernel's layer-0 tile holds only the skip-link channels.  -> (b*n, w_last) or None when unsupported."""
    require_cuda(dist, idx, points1, points2)
    if points1 is None:
        return None
    b, n, m, c1, c2 = _fp_shapes(dist, points1, points2)
    w0a, w0b = split_first_layer(ws[0], c2, c1, "fp_wide_pre", pad_b_rows=8)
    z = hoist_gemm(points2.reshape(b * m, c2), w0a)
    return _launch_stack("pn2_fp_mlp_wide_pre", dist, (b, n, m, c1, dist.contiguous(), idx.contiguous(), points1.contiguous(), z),
                         ws, bs, (), (b * n, ws[-1].shape[1]), w0=w0b)


def hip_sa_mlp_wide_pre(xyz, new_xyz, points, idx, ws, bs, pool=True):
    """pn2_sa_mlp_wide with the feature part of the first layer hoisted: zf = points @ W0[feature rows] on the source points.
    ws[0] in the wide kernel's row order [features (c) | xyz (3) | zero pad].  -> (b, m, w_last) or None when unsupported."""
    require_cuda(xyz, new_xyz, points, idx)
    b, n, _ = xyz.shape
    m, ns = idx.shape[1], idx.shape[2]
    c = points.shape[2]
    w0f, w0x = split_first_layer(ws[0], c, 3, "sa_wide_pre", pad_b_rows=8)
    zf = hoist_gemm(points.reshape(b * n, c), w0f)
    return _launch_stack("pn2_sa_mlp_wide_pre", xyz, (b, n, m, ns, xyz.contiguous(), new_xyz.contiguous(), zf, idx.contiguous()),
                         ws, bs, (int(bool(pool)),), _sa_out_shape(idx, ws[-1].shape[1], pool), w0=w0x)


def hip_fp_mlp_fused(dist, idx, points1, points2, ws, bs):
    """[three_interpolate(points2) | points1] -> up to two dense layers in ONE kernel (pn2_fp_mlp_fused);
    returns (b*n, w_last) or None when the library reports the configuration as unsupported."""
    require_cuda(dist, idx, points1, points2)
    b, n, m, c1, c2 = _fp_shapes(dist, points1, points2)
    p1 = None if points1 is None else points1.contiguous()
    return _launch_stack("pn2_fp_mlp_fused", dist, (b, n, m, c1, c2, dist.contiguous(), idx.contiguous(), p1, points2.contiguous()),
                         ws, bs, (), (b * n, ws[-1].shape[1]))


_zero_bias = {}
HOIST_GEMM_WIDE = False  # A/B: the hoisted products on pn2_mlp_wide instead of pn2_linear (measured: 17.4 vs 13.9 us at 4096 x 256 -> 256, 14.4 vs 13.3 at 16384 x 128 -> 128)


def hoist_gemm(x2d, w):
    """z = x2d @ w (no bias, no activation): the hoisted first-layer products.  4096 .. 65536 rows of width 128 / 256 / 512
    run on the wide-layer kernel (pn2_mlp_wide, single layer), everything else on pn2_linear."""
    rows, cin = x2d.shape
    cout = w.shape[1]
    if HOIST_GEMM_WIDE and 4096 <= rows <= 65536 and cout in (128, 256, 512) and cin % 8 == 0:
        key = (cout, str(w.device))
        zb = _zero_bias.get(key)
        if zb is None:
            zb = _zero_bias[key] = torch.zeros(cout, dtype=torch.float32, device=w.device)
        y = hip_mlp_wide(x2d.contiguous(), [w], [zb], relu_last=False)
        if y is not None:
            return y
    return hip_linear(x2d, w, None, relu=False)


def split_first_layer(w2, c2, c1, key, pad_b_rows=None):
    """(W1a, W1b) = rows [0, c2) and [c2, c2 + c1) of a folded first-layer weight (>= c2 + c1 rows, cout) as contiguous
    tensors (the part whose product is hoisted / the part that stays in the kernel); W1b zero-padded to a multiple of
    pad_b_rows rows when given.  Cached with the folded weight they come from."""
    st = get_default_store()

    def make():
        w1b = w2[c2:c2 + c1] if c1 > 0 else None
        if w1b is not None and pad_b_rows and c1 % pad_b_rows:
            w1b = F.pad(w1b, (0, 0, 0, pad_b_rows - c1 % pad_b_rows))
        return w2[:c2].contiguous(), (None if w1b is None else w1b.contiguous())
    return st.folded((_full_name("split"), key, c2, c1, pad_b_rows), [w2], make)


def hip_fp_mlp_fused_pre(dist, idx, points1, points2, ws, bs, schedule=None):
    """The FP block with the first layer's product hoisted out by linearity (pn2_fp_mlp_fused_pre):
    interp(points2) @ W1a == interp(points2 @ W1a), and Z = points2 @ W1a has the m KNOWN rows per cloud instead of the n
    unknown ones (8x fewer at every level of semantic.json).  Z is one pn2_linear call (no bias, no activation); the fused
    kernel blends three gathered rows of Z straight into its layer-1 accumulators and only the skip-link channels still
    go through the MFMA.  ws[0] = the folded first-layer weight ((c2 + c1 [+ pad]) x w1), 2 or 3 layers, all <= 128 wide.
    schedule (tests, A/B): 0 = the lockstep kernel, 1 = the software-pipelined one (pn2_fp_mlp_fused_pre_schedule); None = the
    library's choice.  Same bits either way.
    Returns (b*n, w_last), or None when the library reports the configuration as unsupported."""
    require_cuda(dist, idx, points1, points2)
    b, n, m, c1, c2 = _fp_shapes(dist, points1, points2)
    L = len(ws)
    if L < 2 or L > 3 or any(w.shape[1] % 32 or w.shape[1] > 128 for w in ws):
        return None
    w1a, w1b = split_first_layer(ws[0], c2, c1, "fp_pre")
    z = hoist_gemm(points2.reshape(b * m, c2), w1a)  # (b*m, w1): the hoisted product
    # the skip link may be a column block of a wider batch (model.get_sa_fp_features: the rgb half of point_cloud): read in place
    p1, ld1 = (None, 0) if points1 is None else rows_in_place(points1)
    if schedule is not None and p1 is not None:
        p1, ld1 = p1.contiguous(), c1
    lead = (b, n, m, c1, dist.contiguous(), idx.contiguous(), p1)
    name, after = "pn2_fp_mlp_fused_pre", ()
    if schedule is not None:
        name, after = "pn2_fp_mlp_fused_pre_schedule", (int(schedule),)
    elif p1 is not None and ld1 != c1:
        name, lead = "pn2_fp_mlp_fused_pre_ld", lead + (ld1,)
    return _launch_stack(name, dist, lead + (z,), ws, bs, (), (b * n, ws[-1].shape[1]), w0=w1b, after=after)  # w1b: None when c1 == 0


def hip_linear_narrow(x2d, w, b=None):
    """y = x2d @ w (+ b) for a layer of at most 16 outputs (the 9-class head) in ONE streaming launch (pn2_linear_narrow);
    None when the library reports the shape as unsupported (the caller pads to an MFMA tile)."""
    require_cuda(x2d, w, b)
    rows, cin = x2d.shape
    cout = w.shape[1]
    if cout > 16 or cin % 4 != 0 or x2d.dtype != torch.float32:
        return None
    x2d = x2d.contiguous()
    y = torch.empty((rows, cout), dtype=torch.float32, device=x2d.device)
    ok = launch("pn2_linear_narrow", x2d, rows, cin, cout, ptr(x2d), ptr(w.contiguous()), ptr(None if b is None else b.contiguous()),
                ptr(y), may_refuse=True)
    return y if ok else None


def hip_matmul(x2d, w):
    """y = x2d @ w on pn2_linear (no bias, no activation) -- the forward GEMM of the training path.  Output widths that
    are not a multiple of 32 run on pn2_linear_narrow (<= 16 outputs: the 9-class head) or with zero-padded weight columns,
    sliced back."""
    cin, cout = w.shape
    if cout <= 16:
        y = hip_linear_narrow(x2d, w)
        if y is not None:
            return y
    if cout % 32 != 0:
        wp = F.pad(w, (0, 32 - cout % 32)).contiguous()
        return hip_linear(x2d, wp, None, relu=False)[:, :cout].contiguous()
    return hip_linear(x2d, w.contiguous(), None, relu=False)


# ---- the training layer path: its A/B switches and thresholds (tests and tools set them as attributes of this module; no path is
# retired -- the off paths are the witnesses the tests compare against).  DESIGN.md section 5 names the parts below. ------------
USE_GEMM_BN_STATS = True  # batch statistics from the forward GEMM's epilogue (set False: separate pass over y; tests / A-B)
# The one-block launches that used to follow every producer of batch-norm sums (fold the slot copies; derive scale / shift resp. the
# gradient constants) are done by the producer's LAST WORKGROUP (csrc/pn2_common.h pn2_bn_finish): a layer inside a stack is one
# launch forward (GEMM + statistics + constants) and two backward (data gradient + finish of the layer below; weight gradient).
# False: the separate launches (A/B, tests).
USE_BN_FINISH_IN_PRODUCER = True
# cross-layer link: the first batch-norm reduction of layer i rides in the data-gradient GEMM of layer i+1.
# When the output z of a dense+BN(+ReLU) layer is consumed by exactly one other such layer, the gradient dz reaching the
# batch norm is the dX of that consumer's data-gradient GEMM.  pn2_linear_dgrad_bn_grad_stats forms the two per-channel
# sums of the batch-norm gradient (sum g, sum g * xhat) from its accumulator tiles, so the producer's backward skips the
# reduction pass over (dz, y) (pn2_bn_relu_backward_mode, BN_WS_SUMMED).  The link is keyed by the storage address of z and checked
# again in the backward: only when the tensor arriving as dz IS the linked GEMM's output (a second consumer makes autograd
# hand over a sum in a new tensor) is the shortcut taken.
USE_DGRAD_BN_STATS = True
# deferred normalisation: layer i publishes (scale, shift) and hands its PRE-normalisation output y to layer i+1
# (pn2_bn_relu_forward_deferred); layer i+1's forward GEMM and weight gradient apply relu(fma(y, scale, shift)) while they
# load y (pn2_linear_bn_stats_xf, pn2_linear_wgrad_accumulate_xf): the normalised activation is never written or re-read.
# Decided by the module code (conv2d(..., defer_bn=True)) for layers whose output feeds exactly the next conv2d of the stack.
USE_BN_ON_LOAD = True
# batch-norm gradient applied on load (round 6): the gradient dy LEAVING a layer's batch norm is only ever read by that
# layer's own data and weight gradient GEMMs, so it is not written: pn2_bn_grad_constants folds the two reduction sums into six
# per-channel constants (+ dgamma, dbeta) and pn2_linear_dgrad_gx / pn2_linear_wgrad_gx form dy from (y, dz) while they load
# their operand -- bn_grad_apply_kernel's pass (read dz, y; write dy) and the two re-reads of dy are gone, and behind the fused
# max pool the (rows, c) gradient never exists at all.  Same float expressions as the materialised form: both hand the GEMMs the
# same bits (tests/test_train_gpu.py::test_bn_grad_on_load_equals_the_materialised_form).
USE_BN_GRAD_ON_LOAD = True
# behind the fused max pool the first backward reduction is taken from the pooled tensors (rows / 32 entries per channel: the
# gradient is non-zero only on the rows attaining a maximum) instead of a pass over y (A/B, tests)
USE_POOLED_BN_REDUCE = True
USE_FUSED_BWD_NARROW = True  # 32 / 64-channel layers: data and weight gradient in one launch, (y, dz) read once (A/B, tests)
USE_SA_FIRST_LAYER_FUSED = True  # SA module, few point channels: front end + first conv + statistics in one launch (A/B, tests)
USE_HOISTED_TRAIN = True  # first layer of SA2-SA4 / FP4 with its feature half applied to the source rows (A/B, tests)
# (FP1-FP3, whose skip link is a wide SA feature tensor that needs a GEMM of its own, keep the concatenated form: the hoisted
# variant was built and measured slower -- 4.13 vs 4.05 ms per step, DESIGN.md section 9 -- and removed in round 4.)
USE_HOIST_BN_STATS = True  # ... and its batch statistics (+ fold + constants) taken by the launch that writes it (A/B, tests)
# (from 32768 rows on: below, the epilogue's tail -- 2 * cout fp64 atomics per workgroup, the ticket, the fold of 64 slot copies
#  by one workgroup -- costs more than the statistics pass it replaces: 8192 x 256: 19 vs 15 us, tools/hoist_stats_ab.py)
HOIST_BN_STATS_MIN_ROWS = 32768
USE_HOISTED_MSG_TRAIN = True  # pointnet_sa_module_msg(geometry=...) in training: all scales' first layers hoisted together (A/B, tests)
MSG_HOIST_MAX_SCALES = 4      # scales one pn2_sa_hoist_rows_multi_bn / pn2_scatter_plan_apply_multi launch takes


def _bn_scratch(c, device, zeroed=False):
    """batch-norm accumulators (pn2_bn_workspace_bytes(c) bytes) and their state (BN_WS_*): a slice of the step's zero arena when
    there is one; else a fresh zero fill (zeroed: for a launch that adds to them) or uncleared memory"""
    nbytes = lib.pn2_bn_workspace_bytes(c)
    arena = get_default_store().zero_arena
    v = arena.take(nbytes) if arena is not None else None
    if v is not None:
        return v, BN_WS_ZEROED
    if zeroed:
        return torch.zeros(nbytes // 8, dtype=torch.float64, device=device), BN_WS_ZEROED
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device), BN_WS_UNCLEARED


def _bn_consts_out(c, device):
    """uninitialised (save_mean, save_invstd, scale, shift) for a launch that publishes a deferred batch norm's constants"""
    save_mean = torch.empty(c, dtype=torch.float32, device=device)
    return save_mean, torch.empty_like(save_mean), torch.empty_like(save_mean), torch.empty_like(save_mean)


def _matmul_bn_stats(entry, x2d, w, ws, *tail):
    """y = x2d @ w on one of the pn2_linear_bn_stats* entry points: they share the argument head (rows, cin, cout, x, w, y, ws,
    bytes of ws) and differ in `tail`"""
    require_cuda(x2d, w)
    rows, cin = x2d.shape
    cout = w.shape[1]
    y = torch.empty((rows, cout), dtype=torch.float32, device=x2d.device)
    launch(entry, x2d, rows, cin, cout, ptr(x2d.contiguous()), ptr(w.contiguous()), ptr(y), ptr(ws), nbytes(ws), *tail)
    return y


def hip_matmul_bn_stats(x2d, w, ws):
    """y = x2d @ w on pn2_linear_bn_stats: the GEMM also leaves the column sums of y and y^2 in the ZEROED batch-norm
    workspace `ws` (pn2_bn_workspace_bytes(cout) bytes), which is then BN_WS_SUMMED.  cout % 32 == 0."""
    return _matmul_bn_stats("pn2_linear_bn_stats", x2d, w, ws)


def hip_matmul_bn_stats_xf(x_raw, w, ws, sc, sh, relu):
    """hip_matmul_bn_stats on relu?(fma(x_raw, sc, sh)) formed while the operand is staged (pn2_linear_bn_stats_xf)"""
    return _matmul_bn_stats("pn2_linear_bn_stats_xf", x_raw, w, ws, ptr(sc), ptr(sh), int(relu))


def hip_matmul_bn_stats_fin(x2d, w, ws, xf, finish, gamma=None, beta=None, b=None, decay=0.0, running_mean=None, running_var=None):
    """hip_matmul_bn_stats (xf None) / hip_matmul_bn_stats_xf (xf = (scale, shift, relu)) whose last workgroup also folds the
    statistics (finish 1) or folds them and publishes the deferred batch norm's constants (finish 2, pn2_linear_bn_stats_fin).
    -> y, (save_mean, save_invstd, scale, shift) or None"""
    consts = _bn_consts_out(w.shape[1], x2d.device) if finish == 2 else None
    sc, sh, xrelu = xf if xf is not None else (None, None, 0)
    y = _matmul_bn_stats("pn2_linear_bn_stats_fin", x2d, w, ws, ptr(sc), ptr(sh), int(xrelu), int(finish), ptr(gamma), ptr(beta),
                         ptr(b), BN_EPSILON, float(decay), ptr(running_mean), ptr(running_var),
                         *map(ptr, consts or (None, None, None, None)))
    return y, consts


def hip_linear_dgrad(dy, w):
    """dx (rows, cin) = dy (rows, cout) @ w^T with w (cin, cout) as the forward pass holds it (pn2_linear_dgrad)."""
    require_cuda(dy, w)
    rows, cout = dy.shape
    cin = w.shape[0]
    dy = dy.contiguous()
    dx = torch.empty((rows, cin), dtype=torch.float32, device=dy.device)
    launch("pn2_linear_dgrad", dy, rows, cin, cout, ptr(dy), ptr(w.contiguous()), ptr(dx))
    return dx


def _wgrad_out(w, fresh=True):
    """the ZERO-STARTED tensor a kernel accumulates dW into: the parameter's slice of the trainer's (zero-filled) flat gradient, else
    a slice of the step's zero arena, else a fresh zero tensor (fresh False: None)"""
    st = get_default_store()
    dw = st.grad_view(w)
    if dw is None:
        v = st.zero_arena.take(w.numel() * 4) if st.zero_arena is not None else None
        if v is not None:
            dw = v[:w.numel() * 4].view(torch.float32).view_as(w)
        elif fresh:
            dw = torch.zeros_like(w)
    return dw


def _hip_wgrad(x2d, dy, w, xf=None):
    """dW = x2d^T @ dy on pn2_linear_wgrad; the tile is added to with atomics, so it starts from the zero arena when the
    step has one (no memset of its own).  xf = (scale, shift, relu): x2d is the producer's un-normalised output, the
    kernel applies its batch norm while loading (pn2_linear_wgrad_accumulate_xf)."""
    dw = _wgrad_out(w, fresh=xf is not None)
    dims = (x2d.shape[0], w.shape[0], w.shape[1], ptr(x2d), ptr(dy))
    if xf is not None:
        launch("pn2_linear_wgrad_accumulate_xf", w, *dims, ptr(dw), ptr(xf[0]), ptr(xf[1]), int(xf[2]))
    elif dw is not None:
        launch("pn2_linear_wgrad_accumulate", w, *dims, ptr(dw))
    else:  # nothing zero-filled at hand: the entry point that clears the tile itself
        dw = torch.empty_like(w)
        launch("pn2_linear_wgrad", w, *dims, ptr(dw))
    return dw


_ones_cache = {}


def _ones_column(rows, device):
    """(rows, 1) of ones: x operand that turns pn2_linear_wgrad into a column sum (bias gradient)"""
    key = (rows, str(device))
    t = _ones_cache.get(key)
    if t is None:
        _ones_cache.clear()  # one size at a time is enough (the head of the network)
        t = _ones_cache[key] = torch.ones((rows, 1), dtype=torch.float32, device=device)
    return t


def _dense_grads(ctx, x2d, w, dy, b_like):
    """(dx, dw, db) of y = x2d @ w (+ b) from dy, as far as ctx.needs_input_grad asks: dX on pn2_linear_dgrad, dW = x2d^T @ dY and
    db = 1^T @ dY (a column sum) on pn2_linear_wgrad.  b_like: (1, cout), what the bias gradient is shaped (and, for a
    parameter's own storage, placed) like; None: a fresh tile."""
    dx = hip_linear_dgrad(dy, w) if ctx.needs_input_grad[0] else None
    dw = _hip_wgrad(x2d, dy, w) if ctx.needs_input_grad[1] else None
    db = None
    if ctx.has_bias and ctx.needs_input_grad[2]:
        b_like = b_like if b_like is not None else dy.new_empty((1, dy.shape[1]))
        db = _hip_wgrad(_ones_column(dy.shape[0], dy.device), dy, b_like).reshape(-1)
    return dx, dw, db


class _TrainMatmul(torch.autograd.Function):
    """y = x2d @ w (+ b) for the training path's un-normalised layers (the class head); backward: dX on
    pn2_linear_dgrad, dW = x2d^T @ dY on pn2_linear_wgrad (the reduction over all rows, ~8x faster than the library
    GEMM on these tall-skinny shapes), db = 1^T @ dY on the same kernel (a column sum)."""

    @staticmethod
    def forward(ctx, x2d, w, b=None):
        ctx.save_for_backward(x2d, w, *(() if b is None else (b,)))
        ctx.has_bias = b is not None
        if w.shape[1] <= 16:  # the class head: GEMM + bias in one streaming launch
            y = hip_linear_narrow(x2d, w, b)
            if y is not None:
                return y
        y = hip_matmul(x2d, w)
        return y if b is None else y.add_(b)

    @staticmethod
    def backward(ctx, dy):
        x2d, w = ctx.saved_tensors[:2]
        return _dense_grads(ctx, x2d, w, dy.contiguous(), ctx.saved_tensors[2].view(1, -1) if ctx.has_bias else None)


class _TrainDenseRelu(torch.autograd.Function):
    """z = relu(x2d @ w + b): the training path of a layer WITHOUT batch norm (reference tf_util.py:186-204 with bn=False:
    conv -> bias_add -> relu).  Forward: pn2_linear with its bias + ReLU epilogue; backward: pn2_relu_grad (TF's ReluGrad: the
    upstream gradient where the OUTPUT is positive), then the data / weight / bias gradients of _TrainMatmul."""

    @staticmethod
    def forward(ctx, x2d, w, b):
        cin, cout = w.shape
        if cout % 32 != 0:  # pn2_linear's output tiles are 32 wide: zero-padded weight / bias columns, sliced back
            pad = 32 - cout % 32
            z = hip_linear(x2d, F.pad(w, (0, pad)).contiguous(), None if b is None else F.pad(b, (0, pad)).contiguous(),
                           relu=True)[:, :cout].contiguous()
        else:
            z = hip_linear(x2d, w.contiguous(), None if b is None else b.contiguous(), relu=True)
        ctx.save_for_backward(x2d, w, z)
        ctx.has_bias = b is not None
        return z

    @staticmethod
    def backward(ctx, dz):
        x2d, w, z = ctx.saved_tensors
        dz = dz.contiguous()
        dy = torch.empty_like(dz)
        launch("pn2_relu_grad", dz, dz.numel(), ptr(z), ptr(dz), ptr(dy))
        return _dense_grads(ctx, x2d, w, dy, None)


def _train_dense(inputs, w2d, b, relu=False):
    """un-normalised dense layer of the training path (the class head): GEMM, data and weight gradients on the HIP library"""
    cin, cout = w2d.shape
    require_cuda(inputs)
    if inputs.dtype != torch.float32:
        raise TypeError("the training path is float32")
    fn = _TrainDenseRelu if relu else _TrainMatmul
    y = fn.apply(inputs.reshape(-1, cin).contiguous(), w2d.contiguous(), b)
    return y.reshape(list(inputs.shape[:-1]) + [cout])


# ---- cross-layer link (USE_DGRAD_BN_STATS, USE_BN_ON_LOAD) ---------------------------------------------------------------
# Registry of the producer records, keyed by the storage address of the producer's output.  WEAK values: the record is owned by
# the producer's autograd context (ctx.link), so it lives exactly as long as that node of the tape -- a forward pass whose tape
# is dropped (or never built) leaves nothing behind, and an address reused by a later tensor finds no stale record.
_bn_links = weakref.WeakValueDictionary()


class _BnLink:
    """What an un-pooled dense+BN layer leaves for the layer that consumes its output, in three stages."""
    __slots__ = ("shape", "y", "gamma", "beta", "mean", "invstd", "relu", "sc", "sh", "gx",  # the forward record
                 "consumed",                                   # a following layer's forward has applied (sc, sh) on load
                 "ws", "ws_state", "dz_ptr", "dz_keep",        # notes of the consumer's data-gradient GEMM: this layer's two sums
                 "coef", "dgamma", "dbeta",                    # ... and, finish kind 3, the gradient constants it published
                 "__weakref__")

    def __init__(self, shape, y, gamma, beta, mean, invstd, relu, sc=None, sh=None, gx=False):
        """sc / sh: the layer deferred its normalisation, its output IS y.  gx: its backward forms the batch-norm gradient on load --
        the consumer's data-gradient GEMM may then publish the gradient constants itself"""
        self.shape, self.y, self.gamma, self.beta, self.mean, self.invstd = tuple(shape), y, gamma, beta, mean, invstd
        self.relu, self.sc, self.sh, self.gx, self.consumed = bool(relu), sc, sh, bool(gx), False
        self.ws = self.ws_state = self.dz_ptr = self.dz_keep = self.coef = self.dgamma = self.dbeta = None

    def note(self, **left):
        """what a consumer's launch has left for this layer's backward, written once the launch has been accepted"""
        for k, v in left.items():
            setattr(self, k, v)

    def spend(self):
        """this layer's backward runs once: refuse a deferred output that no following conv2d consumed, then drop what the record
        kept alive"""
        if self.sc is not None and not self.consumed:
            # the un-normalised output went somewhere else than into the next dense layer: whatever read it saw wrong values
            raise RuntimeError("a deferred batch-norm output (conv2d(..., defer_bn=True)) was not consumed by a following conv2d")
        self.y = self.gamma = self.beta = self.mean = self.invstd = self.sc = self.sh = None
        self.ws = self.ws_state = self.dz_ptr = self.dz_keep = self.coef = self.dgamma = self.dbeta = None


def can_defer_bn(rows, c, c_next):
    """may a layer of width c over `rows` rows hand its un-normalised output to a following layer of width c_next?
    (Only while a tape is being recorded: the record that tells the next layer what it is reading belongs to the tape.)"""
    return bool(USE_BN_ON_LOAD and USE_DGRAD_BN_STATS and torch.is_grad_enabled() and rows > 2048 and c % 4 == 0
                and c_next % 32 == 0)


def assert_not_deferred(x, what):
    """raise if x is the UN-normalised output of a layer that deferred its batch norm (conv2d(..., defer_bn=True)): only the
    next dense layer of the stack may read such a tensor -- anything else would silently compute on un-normalised values"""
    if x is None or not _bn_links:
        return
    lk = _bn_links.get(x.data_ptr())
    if lk is not None and lk.sc is not None and not lk.consumed and lk.shape == (x.numel() // x.shape[-1], x.shape[-1]):
        raise RuntimeError("a deferred batch-norm output (conv2d(..., defer_bn=True)) reached %s" % what)


def _deferred_producer(x2d):
    lk = _bn_links.get(x2d.data_ptr())
    return lk if (lk is not None and lk.sc is not None and lk.y is not None and lk.shape == tuple(x2d.shape)) else None


def reset_bn_links():
    """forget the producer records of the previous forward pass (model.get_model calls this when training)"""
    _bn_links.clear()


def hip_linear_dgrad_linked(dy, w, link):
    """hip_linear_dgrad whose result is the gradient reaching the batch norm of the layer recorded in `link`: the GEMM also
    leaves that batch norm's two gradient sums in a zeroed workspace (pn2_linear_dgrad_bn_grad_stats) and notes both on the
    record for the producer's backward."""
    if USE_BN_FINISH_IN_PRODUCER and w.shape[1] > 16:
        return _hip_dgrad_fin(dy.contiguous(), None, w, link)
    rows, cin = dy.shape[0], w.shape[0]
    dx = torch.empty((rows, cin), dtype=torch.float32, device=dy.device)
    below, _, notes = _below_args(link, rows, cin, dx, fin=False)
    launch("pn2_linear_dgrad_bn_grad_stats", dy, rows, cin, w.shape[1], ptr(dy), ptr(w.contiguous()), ptr(dx), *below)
    link.note(**notes)
    return dx


def _bn_train_forward(y, b, gamma, beta, running_mean, running_var, decay, relu, pool, stats=None):
    """batch norm (+ReLU, + max over groups of `pool` rows) of a layer output y (rows, c); stats: (workspace, BN_WS_* state) from the
    producer of y that has already left the column sums there.  -> z, ties, save_mean, save_invstd"""
    rows, c = y.shape
    ws, state = stats if stats is not None else _bn_scratch(c, y.device)
    pooled = pool > 1
    z = torch.empty((rows // pool, c) if pooled else (rows, c), dtype=y.dtype, device=y.device)
    save_mean = torch.empty(c, dtype=torch.float32, device=y.device)
    save_invstd = torch.empty_like(save_mean)
    ties = None
    head = (rows, c, ptr(y), ptr(gamma), ptr(beta), ptr(b), BN_EPSILON, decay, int(relu))
    if pooled:
        # ties = [tie counts | ysel]: ysel = the pre-normalisation value of the first row attaining each maximum, which lets the
        # backward take its reduction from the pooled tensors (pn2_bn_grad_constants) instead of a pass over y
        ties = torch.empty((2,) + tuple(z.shape), dtype=y.dtype, device=y.device)
        launch("pn2_bn_relu_forward_pool", y, *head, int(pool), ptr(running_mean), ptr(running_var), ptr(ws), nbytes(ws), state,
               ptr(save_mean), ptr(save_invstd), ptr(z), ptr(ties[0]), ptr(ties[1]))
    else:
        launch("pn2_bn_relu_forward_mode", y, *head, ptr(running_mean), ptr(running_var), ptr(ws), nbytes(ws), state, ptr(save_mean),
               ptr(save_invstd), ptr(z))
    return z, ties, save_mean, save_invstd


def _stats_done(state):
    """the stats_done argument of pn2_bn_relu_forward_deferred / pn2_bn_grad_constants for a (zeroed) workspace in `state`"""
    return int(state >= BN_WS_SUMMED)


def _bn_train_forward_deferred(y, b, gamma, beta, running_mean, running_var, decay, stats=None):
    """the statistics half of _bn_train_forward only (pn2_bn_relu_forward_deferred) -> save_mean, save_invstd, scale, shift"""
    rows, c = y.shape
    ws, state = stats if stats is not None else _bn_scratch(c, y.device, zeroed=True)
    consts = _bn_consts_out(c, y.device)
    launch("pn2_bn_relu_forward_deferred", y, rows, c, ptr(y), ptr(gamma), ptr(beta), ptr(b), BN_EPSILON, decay,
           _stats_done(state), ptr(running_mean), ptr(running_var), ptr(ws), nbytes(ws), *map(ptr, consts))
    return consts


def _bn_tail(y, bn, relu, pool, defer, stats=None, consts=None, gx=False):
    """The batch-norm tail of a training forward, shared by the three Functions below.  y (rows, c): the layer's GEMM output;
    bn = (b, gamma, beta, running_mean, running_var, decay); stats: (workspace, BN_WS_* state) when the producer of y has left
    the column sums; consts: (save_mean, save_invstd, scale, shift) when it has published a deferred batch norm's constants too.
    defer: publish (scale, shift) and hand y over UN-normalised -- only the next dense layer of the stack may consume it, and the
    record is what tells that layer what it reads; else normalise (+ ReLU, + max over groups of `pool` rows).  An un-pooled layer
    is recorded as the possible producer of the next layer's input (_BnLink).
    -> output, record or None, what backward needs: always the _BN_SAVED entries (y, gamma, beta, save_mean, save_invstd, zmax,
    ties) -- zmax / ties None unless pooled -- to be saved in this order (_bn_saved reads them back)."""
    gamma, beta = bn[1], bn[2]
    if defer:
        save_mean, save_invstd, sc, sh = consts if consts is not None else _bn_train_forward_deferred(y, *bn, stats)
        out, ties = y, None
    else:
        out, ties, save_mean, save_invstd = _bn_train_forward(y, *bn, relu, pool, stats)
        sc = sh = None
    link = None
    if USE_DGRAD_BN_STATS and not pool > 1:
        link = _bn_links[out.data_ptr()] = _BnLink(out.shape, y, gamma, beta, save_mean, save_invstd, relu, sc, sh, gx)
    if defer and link is None:
        raise RuntimeError("deferred batch norm needs the producer links (USE_DGRAD_BN_STATS)")
    return out, link, (y, gamma, beta, save_mean, save_invstd, out if pool > 1 else None, ties)


_BN_SAVED = 7


def _bn_saved(saved, at):
    """the _BN_SAVED entries of ctx.saved_tensors from position `at` on, where a forward saved _bn_tail's third result
    -> (y, gamma, beta, save_mean, save_invstd, zmax, ties)"""
    return saved[at:at + _BN_SAVED]


def _param_grad_out(p):
    """where a kernel WRITES the gradient of parameter p: its slice of the trainer's flat gradient, else a fresh tensor"""
    gv = get_default_store().grad_view(p)
    return gv if gv is not None else torch.empty_like(p)


def _link_sums(lk, dz, y):
    """(workspace, BN_WS_* state) holding the two gradient sums of the batch norm recorded in lk -- SUMMED, or FOLDED by the
    consumer's data-gradient GEMM (pn2_linear_dgrad_fin) -- when that GEMM has left them AND dz is its output (a second consumer
    makes autograd hand over a sum in a new tensor); else None: the backward reduces (dz, y) itself"""
    if lk is not None and lk.ws is not None and lk.dz_ptr == dz.data_ptr() and dz.shape == y.shape:
        return lk.ws, lk.ws_state
    return None


def _split_ties(ties, zmax):
    """what the pooled forward saved as `ties` -> (tie counts, ysel or None): _bn_train_forward stacks [tie counts | ysel]"""
    if ties is not None and ties.dim() == zmax.dim() + 1:
        return ties[0], ties[1]
    return ties, None


def _bn_train_backward(dz, y, gamma, beta, save_mean, save_invstd, relu, pool, zmax, ties, lk):
    """gradient of _bn_train_forward on pn2_bn_relu_backward_mode -> dy (rows, c), dgamma, dbeta.  lk: this layer's producer
    record (or None); with _link_sums the reduction pass is skipped."""
    rows, c = y.shape
    dz = dz.contiguous()
    dy = torch.empty_like(y)
    dgamma, dbeta = _param_grad_out(gamma), _param_grad_out(beta)
    ws, state = _link_sums(lk, dz, y) or _bn_scratch(c, y.device)
    if lk is not None:
        lk.spend()
    launch("pn2_bn_relu_backward_mode", y, rows, c, ptr(dz), ptr(y), ptr(gamma), ptr(beta), ptr(save_mean), ptr(save_invstd), int(relu),
           int(pool), ptr(zmax), ptr(_split_ties(ties, zmax)[0]), ptr(ws), nbytes(ws), state, ptr(dy), ptr(dgamma), ptr(dbeta))
    return dy, dgamma, dbeta


def _gx_shape_ok(c, pool):
    """can the batch-norm gradient of a layer of width c, pooled over groups of `pool` rows (0: not pooled), be formed on load
    (USE_BN_GRAD_ON_LOAD)?  The part known in the forward; _gx_usable adds what only the backward sees."""
    return bool(USE_BN_GRAD_ON_LOAD and c % 4 == 0 and 16 < c <= 512 and pool in (0, 32))


def _gx_usable(rows, c, pool, dz, y):
    return bool(_gx_shape_ok(c, pool) and (not pool or rows % 32 == 0)
                and dz.dtype == torch.float32 and dz.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)


def _bn_grad_constants(dz, y, gamma, beta, save_mean, save_invstd, relu, pool, zmax, ties, lk):
    """first half of the on-load batch-norm gradient (pn2_bn_grad_constants) -> coef (6, c), dgamma, dbeta.  lk as in
    _bn_train_backward: the reduction pass is skipped when the consumer's data-gradient GEMM has already left the sums."""
    rows, c = y.shape
    sums = _link_sums(lk, dz, y)
    # ... or even published the constants (finish kind 3)
    ready = (lk.coef, lk.dgamma, lk.dbeta) if (sums is not None and lk.coef is not None) else None
    ws, state = sums or _bn_scratch(c, y.device, zeroed=True)
    if lk is not None:
        lk.spend()
    if ready is not None:
        return ready
    coef = torch.empty((6, c), dtype=torch.float32, device=y.device)
    dgamma, dbeta = _param_grad_out(gamma), _param_grad_out(beta)
    ties, ysel = _split_ties(ties, zmax)
    launch("pn2_bn_grad_constants", y, rows, c, ptr(dz), ptr(y), ptr(gamma), ptr(beta), ptr(save_mean), ptr(save_invstd), int(relu),
           int(pool), ptr(zmax), ptr(ties), ptr(ysel if USE_POOLED_BN_REDUCE else None), _stats_done(state), ptr(ws), nbytes(ws),
           ptr(coef), ptr(dgamma), ptr(dbeta))
    return coef, dgamma, dbeta


def _below_args(link, rows, cin, dx, fin):
    """What a data-gradient GEMM with output dx (rows, cin) is handed to serve the layer below (link: its producer record, or
    None): -> below (8 arguments: that layer's batch norm + a zeroed workspace for its two gradient sums), fin_out (4 arguments,
    fin only: what the GEMM's last workgroup does with the sums -- 1 fold them, 3 publish the gradient constants, dgamma and
    dbeta (link.gx) --), notes: what link.note() writes on the record once the launch has been accepted (None without a link)."""
    if link is None:
        return (None, None, None, None, None, 0, None, 0), (0, None, None, None), None
    pws = _bn_scratch(cin, dx.device, zeroed=True)[0]
    below = (ptr(link.y), ptr(link.gamma), ptr(link.beta), ptr(link.mean), ptr(link.invstd), int(link.relu), ptr(pws), nbytes(pws))
    notes = dict(ws=pws, ws_state=BN_WS_FOLDED if fin else BN_WS_SUMMED, dz_ptr=dx.data_ptr(), dz_keep=dx)
    fin_out = (1, None, None, None)
    if fin and link.gx and _gx_usable(rows, cin, 0, dx, link.y):
        coef = torch.empty((6, cin), dtype=torch.float32, device=dx.device)
        dgamma, dbeta = _param_grad_out(link.gamma), _param_grad_out(link.beta)
        notes.update(coef=coef, dgamma=dgamma, dbeta=dbeta)
        fin_out = (3, ptr(coef), ptr(dgamma), ptr(dbeta))
    return below, fin_out, notes


def _hip_dgrad_fin(dy, gx, w, link):
    """The data gradient dx = dy @ w^T of a dense layer with everything the training path hangs on it (pn2_linear_dgrad_fin):
    dy given, or gx = (y, dz, coef, relu, pool, zmax, ties): formed on load; link: the producer record of the layer below -- its
    two batch-norm gradient sums come from the accumulator tiles, and the GEMM's last workgroup folds them (link.gx False: the
    materialised backward follows) or publishes that layer's gradient constants, dgamma and dbeta (link.gx True)."""
    ref = dy if dy is not None else gx[0]
    rows, cin = ref.shape[0], w.shape[0]
    dx = torch.empty((rows, cin), dtype=torch.float32, device=ref.device)
    below, fin_out, notes = _below_args(link, rows, cin, dx, fin=True)
    if gx is not None:
        y, dz, coef, relu, pool, zmax, ties = gx
        up = (None, ptr(y), ptr(dz), ptr(coef), int(relu), int(pool), ptr(zmax), ptr(ties))
    else:
        up = (ptr(dy), None, None, None, 0, 0, None, None)
    launch("pn2_linear_dgrad_fin", ref, rows, cin, w.shape[1], *up, ptr(w.contiguous()), ptr(dx), *below, *fin_out)
    if link is not None:
        link.note(**notes)
    return dx


def _hip_bwd_fused(x2d, xf, y, dz, coef, relu, pool, zmax, ties, w, link):
    """dx AND dW of a narrow layer in ONE launch (pn2_linear_bwd_fused): what _hip_dgrad_fin + _hip_wgrad_gx return, or None when
    the library reports the shape as unsupported (the caller then launches the two)."""
    rows, cin, cout = y.shape[0], w.shape[0], w.shape[1]
    if not (USE_FUSED_BWD_NARROW and USE_BN_FINISH_IN_PRODUCER and cin in (32, 64) and cout in (32, 64) and rows % 32 == 0
            and x2d.is_contiguous() and x2d.shape[1] == cin):
        return None
    dx = torch.empty((rows, cin), dtype=torch.float32, device=y.device)
    dw = _wgrad_out(w)
    below, fin_out, notes = _below_args(link, rows, cin, dx, fin=True)
    sc, sh, xrelu = xf if xf is not None else (None, None, 0)
    ok = launch("pn2_linear_bwd_fused", y, rows, cin, cout, ptr(x2d), ptr(sc), ptr(sh), int(xrelu), ptr(y), ptr(dz), ptr(coef),
                int(relu), int(pool), ptr(zmax), ptr(ties), ptr(w.contiguous()), ptr(dx), ptr(dw), *below, *fin_out, may_refuse=True)
    if not ok:
        return None
    if link is not None:
        link.note(**notes)
    return dx, dw


def _hip_dgrad_gx(y, dz, coef, relu, pool, zmax, ties, w, link):
    """dx = dy @ w^T with dy formed on load (pn2_linear_dgrad_gx); link: the producer record of the layer below (its two batch-norm
    gradient sums are left in a zeroed workspace and noted on the record, as hip_linear_dgrad_linked does) or None"""
    if USE_BN_FINISH_IN_PRODUCER:
        return _hip_dgrad_fin(None, (y, dz, coef, relu, pool, zmax, ties), w, link)
    rows, cin = y.shape[0], w.shape[0]
    dx = torch.empty((rows, cin), dtype=torch.float32, device=y.device)
    below, _, notes = _below_args(link, rows, cin, dx, fin=False)
    launch("pn2_linear_dgrad_gx", y, rows, cin, w.shape[1], ptr(y), ptr(dz), ptr(coef), int(relu), int(pool), ptr(zmax), ptr(ties),
           ptr(w.contiguous()), ptr(dx), *below)
    if link is not None:
        link.note(**notes)
    return dx


def _hip_wgrad_gx(x2d, xf, y, dz, coef, relu, pool, zmax, ties, w):
    """dW = x2d^T @ dy with dy formed on load (pn2_linear_wgrad_gx); xf as in _hip_wgrad"""
    dw = _wgrad_out(w)
    sc, sh, xrelu = xf if xf is not None else (None, None, 0)
    launch("pn2_linear_wgrad_gx", w, x2d.shape[0], w.shape[0], w.shape[1], ptr(x2d), ptr(sc), ptr(sh), int(xrelu), ptr(y), ptr(dz),
           ptr(coef), int(relu), int(pool), ptr(zmax), ptr(ties), ptr(dw))
    return dw


def _backward_grads(ctx, names, **grads):
    """a backward's return value: one entry per forward argument, None except the gradients given by argument name (names: the
    forward's leading argument names, in order)"""
    out = [None] * len(ctx.needs_input_grad)
    for k, g in grads.items():
        out[names.index(k)] = g
    return tuple(out)


def _sa_first_layer_bn(front, w, bn, defer):
    """_dense_bn_gemm's first arm: the first layer of an SA module with few point channels -- gather + centre + concat + product +
    statistics + their fold / constants in ONE launch (pn2_sa_first_layer_bn); the x2d returned = the grouped input it leaves for
    the weight gradient"""
    xyz, new_xyz, points, idx = front
    b, gamma, beta, running_mean, running_var, decay = bn
    c = w.shape[1]
    bsz, n = xyz.shape[0], xyz.shape[1]
    m, ns = idx.shape[1], idx.shape[2]
    cpts = points.shape[2]
    ws = _bn_scratch(c, xyz.device, zeroed=True)[0]
    y = torch.empty((bsz * m * ns, c), dtype=torch.float32, device=xyz.device)
    x2d = torch.empty((bsz * m * ns, 3 + cpts), dtype=torch.float32, device=xyz.device)
    consts = _bn_consts_out(c, xyz.device) if defer else None
    launch("pn2_sa_first_layer_bn", xyz, bsz, n, m, ns, cpts, c, ptr(xyz), ptr(new_xyz), ptr(points), ptr(idx),
           ptr(w.contiguous()), ptr(y), ptr(x2d), ptr(ws), nbytes(ws), 2 if defer else 1, ptr(gamma), ptr(beta), ptr(b),
           BN_EPSILON, float(decay), ptr(running_mean), ptr(running_var), *map(ptr, consts or (None, None, None, None)))
    return y, x2d, (ws, BN_WS_FOLDED), consts


def _dense_bn_gemm(x2d, w, prev, defer, front, bn):
    """The forward GEMM of a dense+BN layer (_TrainDenseBnRelu).  prev: the producer record of x2d, or None; when that layer
    deferred its batch norm, x2d is its UN-normalised output and the GEMM applies (scale, shift, relu) while loading it.  defer: this
    layer defers its own.  front: _sa_first_layer_bn's operands instead of x2d.  bn as in _bn_tail.
    -> y, x2d, stats = (workspace, BN_WS_* state) once the launch has left the column sums of y there (else None), consts = the
    deferred batch norm's constants when the launch has published them too (else None)"""
    if front is not None:
        return _sa_first_layer_bn(front, w, bn, defer)
    b, gamma, beta, running_mean, running_var, decay = bn
    c = w.shape[1]
    xf = (prev.sc, prev.sh, prev.relu) if (prev is not None and prev.sc is not None) else None
    gemm_stats = xf is not None or (USE_GEMM_BN_STATS and c % 32 == 0)
    if gemm_stats and USE_BN_FINISH_IN_PRODUCER:
        # ONE launch: GEMM (batch norm of the layer below applied on load when it was deferred) + column sums of y + -- in the
        # launch's last workgroup -- their fold and, for a layer that defers its own batch norm, its constants
        ws = _bn_scratch(c, x2d.device, zeroed=True)[0]
        y, consts = hip_matmul_bn_stats_fin(x2d, w, ws, xf, 2 if defer else 1, gamma, beta, b, decay, running_mean, running_var)
        return y, x2d, (ws, BN_WS_FOLDED), consts
    if xf is not None:
        ws = _bn_scratch(c, x2d.device, zeroed=True)[0]
        return hip_matmul_bn_stats_xf(x2d, w, ws, *xf), x2d, (ws, BN_WS_SUMMED), None
    if gemm_stats:
        # the GEMM's epilogue leaves the column sums of y in the batch-norm workspace: no statistics pass over y
        ws = _bn_scratch(c, x2d.device, zeroed=True)[0]
        return hip_matmul_bn_stats(x2d, w, ws), x2d, (ws, BN_WS_SUMMED), None
    return hip_matmul(x2d, w), x2d, None, None


class _TrainDenseBnRelu(torch.autograd.Function):
    """relu?(batch_norm(x2d @ w + b)) [-> max over groups of `pool` rows] for the training path, with the
    normalisation on the HIP library: forward = GEMM (_dense_bn_gemm) -> batch norm (_bn_tail: fp64 batch moments, normalise + ReLU
    [+ max pool: the un-pooled activation is never written]; the pre-BN bias only moves the mean, so it is folded into
    the moving average instead of being added); backward = pn2_bn_relu_backward (pool / ReLU masks, dgamma, dbeta, dy)
    -> dX = dY @ w^T, dW on pn2_linear_wgrad.  Replaces nine elementwise / reduction kernels per layer."""
    _ARGS = ("x2d", "w", "b", "gamma", "beta")

    @staticmethod
    def forward(ctx, x2d, w, b, gamma, beta, running_mean, running_var, decay, relu, pool, defer, front=None):
        c = w.shape[1]
        pooled = pool > 1
        # producer of this layer's input (if it was an un-pooled dense+BN layer of this forward pass)
        prev = _bn_links.get(x2d.data_ptr()) if (USE_DGRAD_BN_STATS and x2d is not None) else None
        prev = prev if (prev is not None and prev.y is not None and prev.shape == tuple(x2d.shape)) else None
        xf = prev is not None and prev.sc is not None  # x2d is the producer's UN-normalised output
        defer = defer and not pooled and any(ctx.needs_input_grad)  # no tape node, nobody to keep the record: normalise here
        #                                    (the callers also drop the request when no tape is being recorded at all)
        if xf and c % 32 != 0:
            raise RuntimeError("a deferred batch-norm output reached a layer that cannot apply it")
        bn = (b, gamma, beta, running_mean, running_var, decay)
        y, x2d, stats, consts = _dense_bn_gemm(x2d, w, prev, defer, front, bn)
        if xf:
            prev.consumed = True
        ctx.xf = (prev.sc, prev.sh, bool(prev.relu)) if xf else None
        ctx.relu, ctx.pool = bool(relu), int(pool)
        ctx.prev = prev if (prev is not None and w.shape[1] > 16) else None
        # gx: what backward will do with an un-pooled layer's gradient -- the consumer of this layer's record needs to know
        out, ctx.link, saved = _bn_tail(y, bn, relu, pool, defer, stats, consts, gx=not pooled and _gx_shape_ok(c, 0))
        ctx.save_for_backward(x2d, w, *saved)
        return out

    @staticmethod
    def backward(ctx, dz):
        x2d, w = ctx.saved_tensors[:2]
        y, gamma, beta, save_mean, save_invstd, zmax, ties = _bn_saved(ctx.saved_tensors, 2)
        grads = lambda **g: _backward_grads(ctx, _TrainDenseBnRelu._ARGS, **g)  # noqa: E731
        # (b: a constant in front of batch norm has no effect on the output: its gradient is exactly zero -- None, which the
        # trainer's gradient buffer treats as (and keeps at) zero without a fill per layer)
        dz = dz.contiguous()
        if _gx_usable(y.shape[0], y.shape[1], ctx.pool, dz, y):
            # the gradient leaving the batch norm is formed by the two GEMMs while they load (y, dz): never written
            coef, dgamma, dbeta = _bn_grad_constants(dz, y, gamma, beta, save_mean, save_invstd, ctx.relu, ctx.pool, zmax, ties,
                                                     ctx.link)
            dx = None
            pv = ctx.prev if (ctx.prev is not None and ctx.prev.y is not None) else None
            if ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
                both = _hip_bwd_fused(x2d, ctx.xf, y, dz, coef, ctx.relu, ctx.pool, zmax, ties, w, pv)  # narrow layers: one launch
                if both is not None:
                    return grads(x2d=both[0], w=both[1], gamma=dgamma, beta=dbeta)
            if ctx.needs_input_grad[0]:
                dx = _hip_dgrad_gx(y, dz, coef, ctx.relu, ctx.pool, zmax, ties, w, pv)
            dw = _hip_wgrad_gx(x2d, ctx.xf, y, dz, coef, ctx.relu, ctx.pool, zmax, ties, w) if ctx.needs_input_grad[1] else None
            return grads(x2d=dx, w=dw, gamma=dgamma, beta=dbeta)
        dy, dgamma, dbeta = _bn_train_backward(dz, y, gamma, beta, save_mean, save_invstd, ctx.relu, ctx.pool, zmax, ties, ctx.link)
        dx = None
        if ctx.needs_input_grad[0]:
            pv = ctx.prev
            dx = hip_linear_dgrad_linked(dy, w, pv) if (pv is not None and pv.y is not None) else hip_linear_dgrad(dy, w)
        dw = _hip_wgrad(x2d, dy, w, ctx.xf) if ctx.needs_input_grad[1] else None
        return grads(x2d=dx, w=dw, gamma=dgamma, beta=dbeta)


def _train_variables(scope, cin, cout, bn_decay, pool=0):
    """The variables of a dense+BN layer called in training under `scope` (names, shapes, initialisation as tf_util.conv2d), in
    the form the Functions take them -> w (cin, cout), bn = (b, gamma, beta, moving mean, moving variance, decay) as in
    _bn_tail, pool as 0 or > 1"""
    with variable_scope(scope):
        st, w, b, (beta, gamma, mean, var) = _dense_variables(cin, cout, True, (1, 1, cin, cout))
    st.train_epoch += 1
    decay = 0.9 if bn_decay is None else float(bn_decay)  # tf_util.py:571
    return w.reshape(cin, cout), (b, gamma, beta, mean, var, decay), int(pool) if pool and pool > 1 else 0


def conv2d_sa_first_small(xyz, new_xyz, points, idx, num_output_channels, scope, bn_decay=None, pool=0, defer_bn=False):
    """conv2d(sample_and_group's [grouped_xyz - new_xyz | grouped points], ..., bn=True, is_training=True, relu) -- the FIRST layer
    of an SA module whose points carry at most 5 channels and no gradient (the level-0 module's colours) -- without building the
    grouped tensor first: _TrainDenseBnRelu(front=...) on pn2_sa_first_layer_bn.  Same variables as tf_util.conv2d under `scope`.
    -> (b, m, nsample or 1, cout)"""
    cout = int(num_output_channels)
    w, bn, pool = _train_variables(scope, 3 + points.shape[2], cout, bn_decay, pool)
    front = (xyz.detach().contiguous(), new_xyz.detach().contiguous(), points.detach().contiguous(), idx.contiguous())
    z = _TrainDenseBnRelu.apply(None, w, *bn, True, pool, bool(defer_bn) and not pool and torch.is_grad_enabled(), front)
    m, ns = idx.shape[1], idx.shape[2]
    return z.reshape(xyz.shape[0], m, ns // pool if pool else ns, cout)


def _hip_wgrad_into(x2d, dy, dw_rows):
    """dw_rows (a zero-filled row block of a weight-gradient tile) += x2d^T @ dy on pn2_linear_wgrad_accumulate"""
    launch("pn2_linear_wgrad_accumulate", dy, x2d.shape[0], x2d.shape[1], dy.shape[1], ptr(x2d), ptr(dy), ptr(dw_rows))


class _TrainHoistedBnRelu(torch.autograd.Function):
    """First layer of an SA / FP module, training path, with the feature half of the 1x1 conv applied to the SOURCE rows
    (gather / interpolation are linear and commute with it; csrc/pn2_hoist.hip):
        SA: y = (group_point(xyz, idx) - new_xyz) @ W[:3] + (points @ W[3:])[idx]              (pointnet_util.py:39-54,150-156)
        FP: y = three_interpolate(points2 @ W[:c2], idx, w(dist)) + points1 @ W[c2:]             (pointnet_util.py:300-312)
    then batch norm + ReLU (+ max pool) as in _TrainDenseBnRelu (_bn_tail).  The grouped / concatenated tensor is never built, and
    the GEMM, its data gradient and its weight gradient run on n (resp. m) rows instead of m * nsample (resp. n).  Backward:
    dy from the batch-norm kernels; dz = the scatter of dy through the precomputed plan (the same list the gradient of
    group_point / three_interpolate uses); d(points) = dz @ Wb^T, dWb = points^T dz on the source rows; dWa = a^T dy with
    a = the centred coordinates (SA) resp. points1 (FP: at most 8 skip-link channels that carry no gradient -- the colours
    of the level-0 module)."""
    _ARGS = ("src", "w", "b", "gamma", "beta")

    @staticmethod
    def forward(ctx, src, w, b, gamma, beta, running_mean, running_var, decay, relu, pool, kind, g0, g1, g2, plan, defer):
        bsz, nsrc, c = src.shape
        cout = w.shape[1]
        src2d = src.reshape(-1, c)
        if kind == "sa":
            xyz, new_xyz, idx = g0, g1, g2
            m, ns = idx.shape[1], idx.shape[2]
            wa, wb = w[:3], w[3:]
            rows_b = m * ns
        else:
            dist, idx, points1 = g0, g1, g2
            n, c1 = points1.shape[1], points1.shape[2]
            wb, wa = w[:c], w[c:]
            rows_b = n
        z = hip_matmul(src2d, wb)  # (b * nsrc, cout)
        y = torch.empty((bsz * rows_b, cout), dtype=torch.float32, device=src.device)
        defer = defer and not pool > 1 and any(ctx.needs_input_grad)  # as _TrainDenseBnRelu
        # the deferred batch norm's statistics (+ their fold and the constants) ride in the launch that writes y
        # (from HOIST_BN_STATS_MIN_ROWS rows on, see there)
        fused_stats = bool(defer and USE_HOIST_BN_STATS and USE_BN_FINISH_IN_PRODUCER and bsz * rows_b >= HOIST_BN_STATS_MIN_ROWS)
        consts, bn_args = None, ()
        if fused_stats:
            ws = _bn_scratch(cout, src.device, zeroed=True)[0]
            consts = _bn_consts_out(cout, src.device)
            bn_args = (ptr(ws), nbytes(ws), 2, ptr(gamma), ptr(beta), ptr(b), BN_EPSILON, float(decay),
                       ptr(running_mean), ptr(running_var), *map(ptr, consts))
        if kind == "sa":
            a = torch.empty((bsz * rows_b, 3), dtype=torch.float32, device=src.device)
            launch("pn2_sa_hoist_rows_bn" if fused_stats else "pn2_sa_hoist_rows", src, bsz, nsrc, m, ns, cout, ptr(xyz), ptr(new_xyz),
                   ptr(idx), ptr(z), ptr(wa), ptr(y), ptr(a), *bn_args)
        else:
            a = points1.reshape(-1, c1)
            if c1 > 8:
                raise ValueError("the hoisted FP front end takes at most 8 skip-link channels")
            launch("pn2_fp_hoist_rows_bn" if fused_stats else "pn2_fp_hoist_rows", src, bsz, n, nsrc, c1, cout, ptr(dist), ptr(idx),
                   ptr(a), ptr(z), ptr(wa), ptr(y), *bn_args)
        ctx.relu, ctx.pool, ctx.kind, ctx.dims = bool(relu), int(pool), kind, (bsz, nsrc, rows_b, c)
        out, ctx.link, saved = _bn_tail(y, (b, gamma, beta, running_mean, running_var, decay), relu, pool, defer, consts=consts)
        ctx.save_for_backward(src2d, w, a, plan, *saved)
        return out

    @staticmethod
    def backward(ctx, dz):
        src2d, w, a, plan = ctx.saved_tensors[:4]
        y, gamma, beta, save_mean, save_invstd, zmax, ties = _bn_saved(ctx.saved_tensors, 4)
        bsz, nsrc, rows_b, c = ctx.dims
        cout = w.shape[1]
        dy, dgamma, dbeta = _bn_train_backward(dz, y, gamma, beta, save_mean, save_invstd, ctx.relu, ctx.pool, zmax, ties, ctx.link)
        sa = ctx.kind == "sa"
        wa, wb = (w[:3], w[3:]) if sa else (w[c:], w[:c])
        from .pointnet_util import _scatter_plan_apply
        dzs = _scatter_plan_apply(plan, dy.view(bsz, rows_b, cout), 0, cout, rows_b if sa else 3 * rows_b, 1 if sa else 3, nsrc)
        dzs2d = dzs.view(-1, cout)
        dsrc = hip_linear_dgrad(dzs2d, wb).view(bsz, nsrc, c) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dw = _wgrad_out(w)
            dwa, dwb = (dw[:3], dw[3:]) if sa else (dw[c:], dw[:c])
            _hip_wgrad_into(src2d, dzs2d, dwb)
            _hip_wgrad_into(a, dy, dwa)
        return _backward_grads(ctx, _TrainHoistedBnRelu._ARGS, src=dsrc, w=dw, gamma=dgamma, beta=dbeta)


def conv2d_hoisted_first(kind, src, geo, plan, cin, num_output_channels, scope, bn_decay=None, pool=0, defer_bn=False):
    """conv2d(concat-of-a-gathered-tensor, ..., bn=True, is_training=True, activation relu) -- the FIRST layer of an SA
    (kind "sa": geo = (xyz, new_xyz, idx)) or FP (kind "fp": geo = (dist, idx, points1)) module -- without building the
    gathered tensor: _TrainHoistedBnRelu.  Same variables (names, shapes, initialisation) as tf_util.conv2d under `scope`;
    cin = width of the tensor the reference convolves (3 + c resp. c2 + c1).
    -> (b, m, nsample or nsample/pool, cout) resp. (b, n, 1, cout)."""
    cout = int(num_output_channels)
    w, bn, pool = _train_variables(scope, cin, cout, bn_decay, pool)
    z = _TrainHoistedBnRelu.apply(src.contiguous(), w, *bn, True, pool, kind, geo[0].contiguous(), geo[1].contiguous(),
                                  geo[2].contiguous(), plan, bool(defer_bn) and not pool and torch.is_grad_enabled())
    if kind == "sa":
        m, ns = geo[2].shape[1], geo[2].shape[2]
        return z.reshape(src.shape[0], m, ns // pool if pool else ns, cout)
    return z.reshape(src.shape[0], geo[2].shape[1], 1, cout)


# _TrainHoistedMsgBnRelu's argument list: _MSG_HEAD, then one _MsgScale record per scale, flattened (autograd takes tensors as
# arguments of their own); backward returns one gradient per entry in the same layout
_MSG_HEAD = ("src", "xyz", "new_xyz", "decay", "pools", "defers")
_MsgScale = namedtuple("_MsgScale", "w b gamma beta running_mean running_var idx plan", defaults=(None,) * 8)


def _msg_pack(scales):
    return [v for sc in scales for v in sc]


def _msg_unpack(per):
    n = len(_MsgScale._fields)
    return [_MsgScale(*per[i:i + n]) for i in range(0, len(per), n)]


class _TrainHoistedMsgBnRelu(torch.autograd.Function):
    """The first layers of ALL scales of pointnet_sa_module_msg (pointnet_util.py:219-282), training path, hoisted together: every
    scale gathers from the same source cloud, so the feature halves of their first 1x1 convs are ONE GEMM of the n source rows
    against the column-concatenated weights,
        z = points @ [Wf_0 | Wf_1 | ...],     y_s = z[idx_s, its columns] + (group_point(xyz, idx_s) - new_xyz) @ Wx_s
    (one pn2_linear, one pn2_sa_hoist_rows_multi_bn that also takes every scale's batch statistics), then per scale batch norm +
    ReLU (+ max over K, or deferred) as in _TrainHoistedBnRelu (_bn_tail).  The variables keep the reference's [features | xyz] row
    order (:259): Wf_s = w_s[:C], Wx_s = w_s[C:].  Backward: dy_s from the batch-norm kernels; ONE pn2_scatter_plan_apply_multi into
    the shared dz (b, n, sum cout); d(points) = dz @ Wf_all^T -- the GEMM's reduction adds the scales' contributions --; ONE weight
    gradient points^T dz whose column blocks are the feature rows of the variables' gradients; dWx_s = gxyz_s^T dy_s.
    Arguments after `defers`: per scale a _MsgScale (w (C + 3, cout), b, gamma, beta, running_mean, running_var, idx, plan).
    -> one tensor per scale: (b * m * K_s, cout_s), or (b * m, cout_s) behind the fused max (pools[s] = K_s > 1)."""

    @staticmethod
    def forward(ctx, src, xyz, new_xyz, decay, pools, defers, *per):
        scales = _msg_unpack(per)
        nsc = len(scales)
        bsz, nsrc, c = src.shape
        src2d = src.reshape(-1, c)
        col = lambda k: [getattr(sc, k) for sc in scales]  # noqa: E731
        ws_, idxs = col("w"), col("idx")
        m = idxs[0].shape[1]
        ks = [int(i.shape[2]) for i in idxs]
        couts = [int(w.shape[1]) for w in ws_]
        cols = [sum(couts[:s]) for s in range(nsc)]
        wf_all = torch.cat([w[:c] for w in ws_], dim=1) if nsc > 1 else ws_[0][:c].contiguous()
        z = hip_matmul(src2d, wf_all)  # (b * nsrc, sum cout)
        needs = any(ctx.needs_input_grad)
        defers = [bool(d) and not pools[s] and needs for s, d in enumerate(defers)]  # as _TrainDenseBnRelu
        fin = bool(USE_BN_FINISH_IN_PRODUCER)
        finish = [(2 if d else 1) if fin else 0 for d in defers]
        left = BN_WS_FOLDED if fin else BN_WS_SUMMED  # state of a scale's workspace after the launch (finish 1 / 0)
        ys = [torch.empty((bsz * m * k, co), dtype=torch.float32, device=src.device) for k, co in zip(ks, couts)]
        gx = [torch.empty((bsz * m * k, 3), dtype=torch.float32, device=src.device) for k in ks]
        wss = [_bn_scratch(co, src.device, zeroed=True)[0] for co in couts]
        consts = [_bn_consts_out(co, src.device) if f == 2 else None for co, f in zip(couts, finish)]
        wxs = [w[c:] for w in ws_]
        launch("pn2_sa_hoist_rows_multi_bn", src, nsc, bsz, nsrc, m, z.shape[1], ptr(xyz), ptr(new_xyz), ptr(z), int_array(ks),
               int_array(couts), int_array(cols), ptr_table(idxs), ptr_table(wxs), ptr_table(ys), ptr_table(gx), ptr_table(wss),
               u64_array([nbytes(w_) for w_ in wss]), int_array(finish), ptr_table(col("gamma")), ptr_table(col("beta")),
               ptr_table(col("b")), BN_EPSILON, float(decay), ptr_table(col("running_mean")), ptr_table(col("running_var")),
               *(ptr_table([cs[k] if cs else None for cs in consts]) for k in range(4)))
        outs, saved, links = [], [src2d, wf_all], []
        for s, sc in enumerate(scales):
            out, lk, kept = _bn_tail(ys[s], (sc.b, sc.gamma, sc.beta, sc.running_mean, sc.running_var, decay), True, int(pools[s]),
                                     defers[s], (wss[s], left), consts[s])
            saved += [sc.w, gx[s], sc.plan, *kept]
            outs.append(out)
            links.append(lk)
        ctx.save_for_backward(*saved)
        ctx.links, ctx.pools, ctx.dims, ctx.cols = links, [int(p) for p in pools], (bsz, nsrc, m, c), cols
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dzs):
        saved = ctx.saved_tensors
        src2d, wf_all = saved[:2]
        bsz, nsrc, m, c = ctx.dims
        nsc = len(ctx.pools)
        ws_, dys, gxs, plans, grads = [], [], [], [], []
        for s in range(nsc):
            at = 2 + s * (3 + _BN_SAVED)
            w, a, plan = saved[at:at + 3]
            y, gamma, beta, save_mean, save_invstd, zmax, ties = _bn_saved(saved, at + 3)
            dy, dgamma, dbeta = _bn_train_backward(dzs[s], y, gamma, beta, save_mean, save_invstd, True, ctx.pools[s], zmax, ties,
                                                   ctx.links[s])
            ws_.append(w); dys.append(dy); gxs.append(a); plans.append(plan)
            grads.append(dict(gamma=dgamma, beta=dbeta))
        couts = [int(w.shape[1]) for w in ws_]
        total = wf_all.shape[1]
        dzall = torch.empty((bsz, nsrc, total), dtype=torch.float32, device=src2d.device)
        launch("pn2_scatter_plan_apply_multi", dzall, nsc, bsz, nsrc, total, int_array([dy.shape[0] // bsz for dy in dys]),
               int_array([1] * nsc), int_array(couts), int_array(ctx.cols), ptr_table(dys), int_array(couts), ptr_table(plans),
               u64_array([p.numel() for p in plans]), ptr(dzall))
        dz2d = dzall.view(-1, total)
        dsrc = hip_linear_dgrad(dz2d, wf_all).view(bsz, nsrc, c) if ctx.needs_input_grad[0] else None
        if any(need.w for need in _msg_unpack(ctx.needs_input_grad[len(_MSG_HEAD):])):
            dwf = torch.empty((c, total), dtype=torch.float32, device=src2d.device)
            launch("pn2_linear_wgrad", dz2d, src2d.shape[0], c, total, ptr(src2d), ptr(dz2d), ptr(dwf))
            for s in range(nsc):
                dw = _wgrad_out(ws_[s])
                dw[:c].copy_(dwf[:, ctx.cols[s]:ctx.cols[s] + couts[s]])  # the column block -> the feature rows of the variable's gradient
                _hip_wgrad_into(gxs[s], dys[s], dw[c:])
                grads[s]["w"] = dw
        return _backward_grads(ctx, _MSG_HEAD, src=dsrc)[:len(_MSG_HEAD)] + tuple(_msg_pack(_MsgScale(**g) for g in grads))


def conv2d_hoisted_first_msg(points, xyz, new_xyz, idxs, plans, num_output_channels, scopes, bn_decay=None, pools=None,
                             defer_bn=None):
    """conv2d(concat[group_point(points, idx_s) | grouped_xyz_s - new_xyz], ..., bn=True, is_training=True, relu) for every scale
    s of pointnet_sa_module_msg at once, without building the grouped tensors: _TrainHoistedMsgBnRelu.  Same variables (names,
    shapes, [features | xyz] row order, initialisation) as tf_util.conv2d under scopes[s]; pools[s] = nsample for a one-layer
    scale (the max over K is fused), else 0; defer_bn[s]: hand the un-normalised output to the scale's next conv2d.
    -> [(b, m, nsample_s or 1, cout_s)]"""
    nsc = len(idxs)
    if not 1 <= nsc <= MSG_HOIST_MAX_SCALES:
        raise ValueError("conv2d_hoisted_first_msg takes 1..%d scales" % MSG_HOIST_MAX_SCALES)
    cin = points.shape[2] + 3
    pools = [int(p) if p and p > 1 else 0 for p in (pools or [0] * nsc)]
    defers = [bool(d) and not pools[s] and torch.is_grad_enabled() for s, d in enumerate(defer_bn or [False] * nsc)]
    scales = []
    for s in range(nsc):
        w, bn, _ = _train_variables(scopes[s], cin, int(num_output_channels[s]), bn_decay)
        scales.append(_MsgScale(w, *bn[:5], idxs[s].contiguous(), plans[s]))
    decay = bn[5]  # the same for every scale
    outs = _TrainHoistedMsgBnRelu.apply(points.contiguous(), xyz.detach().contiguous(), new_xyz.detach().contiguous(), decay,
                                        tuple(pools), tuple(defers), *_msg_pack(scales))
    b, m = points.shape[0], idxs[0].shape[1]
    return [o.reshape(b, m, 1 if pools[s] else idxs[s].shape[2], int(num_output_channels[s])) for s, o in enumerate(outs)]


def _train_layer(inputs, w2d, b, bnv, bn_decay, relu, pool=0, defer=False):
    """One dense layer of the training path, entirely on the HIP library: inputs (..., cin) -> (..., cout); pool > 1 also
    takes the max over groups of `pool` consecutive entries of the second-to-last axis (..., W, cin) -> (..., W/pool, cout).
    With batch norm: _TrainDenseBnRelu; without: _TrainMatmul (activation None: the class head) or _TrainDenseRelu (bn=False
    layers of the layer API, tf_util.py:186-204).  There is no torch fallback: batch-norm widths beyond 1024, or not a multiple of
    4 above 256, run as independent column blocks on the same kernels.  (tests/torch_layers.py holds the plain-torch reference
    of this function.)"""
    cin, cout = w2d.shape
    pool = int(pool) if pool and pool > 1 else 0
    lead = list(inputs.shape[:-1])
    if pool:
        if lead[-1] % pool:
            raise ValueError("pool must divide the grouped axis")
        lead[-1] //= pool
    require_cuda(inputs)
    if inputs.dtype != torch.float32:
        raise TypeError("the training path is float32")
    if bnv is None:
        if pool:  # the fused max over K lives in the batch-norm kernels; a layer without batch norm is pooled by its caller
            raise ValueError("pool > 1 needs bn=True on the training path (pointnet_sa_module pools bn=False stacks with group_pool)")
        if _deferred_producer(inputs.reshape(-1, cin)) is not None:
            raise RuntimeError("a deferred batch-norm output reached a layer without batch norm")
        return _train_dense(inputs, w2d, b, relu=relu)
    if not (cout <= 1024 and (cout % 4 == 0 or cout <= 256)):
        # A width the batch-norm kernels do not take in one piece (> 1024 channels, or > 256 and not a multiple of 4; the reference's
        # batch_norm_template takes any width, tf_util.py:555-581).  Batch norm, ReLU and the max over K act per channel, so the
        # layer IS the concatenation of independent layers on column blocks of (W, gamma, beta, moving averages): blocks of
        # <= 1024 channels (multiples of 4) and one remainder of <= 256.  Slow -- one GEMM and one set of batch-norm launches per
        # block, a column copy in and a concatenation out -- but every value comes from the same HIP kernels.
        beta, gamma, mean, var = bnv
        cuts, c0 = [], 0
        while cout - c0 > 256 and (cout - c0) % 4 != 0 or cout - c0 > 1024:
            step = min(1024, (cout - c0) // 4 * 4)
            if (cout - c0 - step) > 256 and step < 1024:  # keep the remainder <= 256
                step = (cout - c0 - 256 + 3) // 4 * 4
            cuts.append((c0, c0 + step))
            c0 += step
        cuts.append((c0, cout))
        outs = [_train_layer(inputs, w2d[:, a:e].contiguous(), None if b is None else b[a:e],
                             (beta[a:e], gamma[a:e], mean[a:e], var[a:e]), bn_decay, relu, pool, defer=False) for a, e in cuts]
        return torch.cat(outs, dim=-1)
    beta, gamma, mean, var = bnv
    decay = 0.9 if bn_decay is None else float(bn_decay)  # tf_util.py:571
    z = _TrainDenseBnRelu.apply(inputs.reshape(-1, cin).contiguous(), w2d.contiguous(), b, gamma, beta, mean, var,
                                decay, relu, pool, bool(defer) and not pool and relu and torch.is_grad_enabled())
    return z.reshape(lead + [cout])


def conv2d(inputs, num_output_channels, kernel_size, scope, stride=(1, 1), padding="SAME", data_format="NHWC",
           use_xavier=True, stddev=1e-3, weight_decay=None, activation_fn=torch.relu, bn=False, bn_decay=None,
           is_training=None, pool=0, defer_bn=False, pool_idx=None):
    """1x1 conv over an NHWC tensor (B,H,W,C) = matmul over C (tf_util.py:128-204).
    Only the configuration the SA/FP stack uses is implemented: kernel [1,1],
    stride [1,1], NHWC.  `pool` (extension): max over groups of `pool` rows of W,
    fused in the HIP epilogue on the inference path.  `pool_idx` (extension, inference, pool = 32): the ball query (B,H,32)
    whose rows `inputs` was computed behind -- the layer then runs on the live rows only (hip_linear_pool_packed: same bits),
    on all rows where the library refuses."""
    if list(kernel_size) != [1, 1] or list(stride) != [1, 1] or data_format != "NHWC":
        raise NotImplementedError("only 1x1 / stride 1 / NHWC conv2d is on the SA/FP path")
    if activation_fn not in (torch.relu, None):
        raise NotImplementedError("activation_fn must be relu or None")
    cin = inputs.shape[-1]
    cout = int(num_output_channels)
    with variable_scope(scope):
        if not is_training:
            w2, b2 = folded_dense(cin, cout, bn, (1, 1, cin, cout), pad_to=32)
            y = None
            if pool_idx is not None and pool == 32 and activation_fn is not None:
                y = hip_linear_pool_packed(inputs.reshape(-1, cin), pool_idx, w2, b2)
            if y is None:
                y = hip_linear(inputs.reshape(-1, cin), w2, b2, relu=activation_fn is not None, pool=pool)
            if y.shape[1] != cout:
                y = y[:, :cout]
            lead = list(inputs.shape[:-1])
            if pool and pool > 1:
                lead[-1] //= pool
            return y.reshape(lead + [cout])
        st, w, b, bnv = _dense_variables(cin, cout, bn, (1, 1, cin, cout))
        st.train_epoch += 1
        # defer_bn (extension, training): hand the UN-normalised output to the next conv2d of the stack (see USE_BN_ON_LOAD)
        return _train_layer(inputs, w.reshape(cin, cout), b, bnv, bn_decay, activation_fn is not None, pool,
                            defer=bool(defer_bn) and bn)


def conv1d(inputs, num_output_channels, kernel_size, scope, stride=1, padding="SAME", use_xavier=True,
           stddev=1e-3, weight_decay=None, activation_fn=torch.relu, bn=False, bn_decay=None, is_training=None):
    """kernel-1 conv over (B,N,C) (tf_util.py:54-125): same maths as conv2d on (B,N,1,C)."""
    if kernel_size != 1 or stride != 1:
        raise NotImplementedError("only kernel 1 / stride 1 conv1d is on the SA/FP path")
    cin = inputs.shape[-1]
    cout = int(num_output_channels)
    with variable_scope(scope):
        if not is_training:
            if cout <= 16 and not bn and activation_fn is None:  # the class head (model.py:145-146): one streaming launch
                st, w, b, _ = _dense_variables(cin, cout, False, (1, cin, cout))
                y = hip_linear_narrow(inputs.reshape(-1, cin), w.detach().reshape(cin, cout), b.detach())
                if y is not None:
                    return y.reshape(list(inputs.shape[:-1]) + [cout])
            w2, b2 = folded_dense(cin, cout, bn, (1, cin, cout), pad_to=32)
            y = hip_linear(inputs.reshape(-1, cin), w2, b2, relu=activation_fn is not None)
            if y.shape[1] != cout:
                y = y[:, :cout].contiguous()
            return y.reshape(list(inputs.shape[:-1]) + [cout])
        st, w, b, bnv = _dense_variables(cin, cout, bn, (1, cin, cout))
        st.train_epoch += 1
        y = _train_layer(inputs, w.reshape(cin, cout), b, bnv, bn_decay, activation_fn is not None)
        return y


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep_prob, state):
        x = x.contiguous()
        y = torch.empty_like(x)
        mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        launch("pn2_dropout", x, x.numel(), ptr(x), float(keep_prob), ptr(state), ptr(y), ptr(mask))
        ctx.save_for_backward(mask)
        ctx.keep = float(keep_prob)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        launch("pn2_dropout_grad", dy, dy.numel(), ptr(dy), ptr(mask), ctx.keep, ptr(dx))
        return dx, None, None


def dropout(inputs, is_training, scope, keep_prob=0.5, noise_shape=None):
    """tf_util.py:646-665: active only while training.  The draw is a pure function of (store seed ^ scope, store
    step counter, element index) read from device memory (pn2_dropout): replayable inside a captured hipGraph; the
    trainer advances `store.rng_state[1]` once per step."""
    if not is_training:
        return inputs
    if noise_shape is not None:
        raise NotImplementedError("noise_shape is not used on the SA/FP path")
    require_cuda(inputs)
    st = get_default_store()
    import zlib
    key = _full_name(scope)
    state = st.dropout_state(key, zlib.crc32(key.encode()))
    assert_not_deferred(inputs, "dropout")
    return _Dropout.apply(inputs, keep_prob, state)
