"""ctypes binding of libpn2_hip.so (the C ABI declared in include/pn2_abi.h).

There is deliberately NO fallback: if the HIP library cannot be loaded the
import fails loudly.  The library must be loaded after `import torch` so that it
binds to the HIP runtime torch already mapped (same soname libamdhip64.so.7);
tensors and streams are then shared with torch without copies.

The binding is read from the header (_abi.py): argument types, return types, the PN2_* constants and the benchmark trace's
table all come from its prototypes.  A new entry point is added in include/pn2_abi.h and its .hip file -- and to _STATEFUL
below if it changes caller state beyond its outputs, which no prototype says.  Nothing else changes on the Python side.
"""
import ctypes
import os
import sys

import torch  # noqa: F401  (must precede CDLL: maps torch's libamdhip64.so.7)

from . import _abi, build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
# PN2_HIP_LIBRARY: load another build of the same ABI instead (the tuning build of the A/B scripts under tools/)
LIB_PATH = os.environ.get("PN2_HIP_LIBRARY") or os.path.join(_HERE, "libpn2_hip.so")

c_int, c_float, c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p

ABI = _abi.load(_build.HEADER)
# the entry points (-> int: 0, PN2_E* or a hipError_t): name -> argtypes, in the order of the header
SIGNATURES = {name: f.argtypes for name, f in ABI.functions.items() if f.restype is c_int and name != "pn2_abi_version"}
PN2_EUNSUP = ABI.constants["PN2_EUNSUP"]
# state of a batch-norm workspace when a call arrives: PN2_BN_WS_* of include/pn2_abi.h (the stats_mode argument)
BN_WS_UNCLEARED, BN_WS_ZEROED, BN_WS_SUMMED, BN_WS_FOLDED = (
    ABI.constants["PN2_BN_WS_" + state] for state in ("UNCLEARED", "ZEROED", "SUMMED", "FOLDED"))


def _trace_args():
    """What the benchmark trace decodes besides the numeric arguments: entry point -> (index of nlayers, index of the host widths[]
    array in the argument list -- both None when there is none --, trace key, positions AMONG THE NUMERIC ARGUMENTS to drop).  An
    in-place (row-strided) *_ld call is the dense entry point's kernel: recorded under the dense name with its strides dropped.
    Read off the header's parameter names: `nlayers`, `widths`, and `ld*` for a row stride."""
    table = {}
    for name, f in ABI.functions.items():
        at = {arg: i for i, arg in enumerate(f.argnames)}
        numeric = [arg for arg, t in zip(f.argnames, f.argtypes) if t is not c_void_p]
        drop = tuple(i for i, arg in enumerate(numeric) if arg.startswith("ld"))
        if drop or "nlayers" in at or "widths" in at:
            table[name] = (at.get("nlayers"), at.get("widths"), name[:-3] if name.endswith("_ld") else None, drop)
    return table


_TRACE_ARGS = _trace_args()


class Pn2Error(RuntimeError):
    pass


def _load():
    # Build in-tree with hipcc when the library is missing OR older than its sources (cross-compiles without a GPU);
    # never fall back to CPU code.  One process per GPU may import concurrently (torch.distributed.run): the check
    # and the build run under a file lock, and build.py links to a temporary file that is renamed into place, so no
    # rank can dlopen a half-written library.  An up-to-date library is loaded without touching the tree (it may be
    # read-only to the user who runs it); the lock is taken only when a build may be needed.
    import fcntl
    if not os.environ.get("PN2_HIP_LIBRARY") and _build._stale():
        if not os.access(_HERE, os.W_OK) and os.path.exists(_build.LIB):
            sys.stderr.write("pn2: %s is older than its sources but %s is not writable: loading the library as built\n"
                             % (_build.LIB, _HERE))
        else:
            with open(os.path.join(_HERE, ".build.lock"), "a") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    if _build._stale():  # another process may have built it while this one waited
                        _build.build()
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise ImportError("cannot load the HIP extension %s: %s -- there is no CPU fallback; "
                          "build it with `python open3d-pointnet2-semantic3d_amd/build.py`" % (LIB_PATH, e))
    for name, f in ABI.functions.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library disagree
        fn.argtypes, fn.restype = f.argtypes, f.restype
    if lib.pn2_abi_version() != ABI.constants["PN2_ABI_VERSION"]:
        raise ImportError("libpn2_hip.so ABI version mismatch")
    return lib


_raw = _load()


# entry points that mutate caller state beyond their outputs (moving averages, optimizer slots): never launched twice by the dup hook
_STATEFUL = frozenset({"pn2_bn_relu_forward", "pn2_linear_bn_stats",
                       "pn2_bn_relu_forward_pool", "pn2_bn_relu_forward_deferred", "pn2_linear_bn_stats_xf", "pn2_linear_wgrad_gx",
                       "pn2_linear_wgrad_accumulate_xf", "pn2_bn_grad_constants", "pn2_linear_dgrad_gx", "pn2_linear_dgrad_fin",
                       "pn2_linear_bn_stats_fin", "pn2_bn_relu_forward_mode", "pn2_sa_first_layer_bn", "pn2_sa_hoist_rows_bn", "pn2_fp_hoist_rows_bn", "pn2_sa_hoist_rows_multi_bn", "pn2_linear_bwd_fused", "pn2_linear_dgrad_bn_grad_stats",
                       "pn2_adam_step", "pn2_momentum_step", "pn2_linear_wgrad_accumulate",
                       "pn2_augment", "pn2_frame_sample",  # (advance the caller's counter: a second launch draws other numbers)
                       "pn2_tile_vote", "pn2_tile_vote_scores",  # (add into the caller's votes / scores)
                       "pn2_render_splat"})  # (takes the minimum into the caller's z-buffer, counts into its culled)


class _LibProxy:
    """Attribute proxy over the ctypes library.  When `trace` is a list, every pn2_* launch is
    bracketed by two events on torch's current stream (the stream the kernel is launched on) and
    (name, numeric_args, start_event, end_event) is appended -- bench.py derives per-kernel durations
    and roofline numbers from it.  With trace=None (default) calls go straight through."""

    def __init__(self, raw):
        self._raw = raw
        self.trace = None
        self.dup = ()  # experiment hook: entry points launched twice (marginal-cost ablation, bench.py --dup)

    def __getattr__(self, name):
        fn = getattr(self._raw, name)
        if name not in SIGNATURES:
            return fn

        def call(*args):
            if name in self.dup and name not in _STATEFUL:
                fn(*args)  # a pure function of its inputs: the second launch rewrites the same values
            if self.trace is None:
                return fn(*args)
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            rc = fn(*args)
            e.record()
            ints = [a for a in args if isinstance(a, (int, float))]
            key = name
            if name in _TRACE_ARGS:
                nl_at, w_at, dense, drop = _TRACE_ARGS[name]
                key = dense or name
                ints = [v for i, v in enumerate(ints) if i not in drop]
                if w_at is not None:  # decode the host-side widths[] array for flop accounting
                    wp = ctypes.cast(args[w_at], ctypes.POINTER(c_int))
                    ints += [wp[i] for i in range(args[nl_at])]
            elif name == "pn2_coarse_geometry":  # (b, n0, nlev, npoint[], radius[], nsample[], ...): decode the host arrays
                ints += list(args[3]) + list(args[5])
            self.trace.append((key, tuple(ints), s, e))
            return rc

        call.__name__ = name
        setattr(self, name, call)  # cache
        return call


lib = _LibProxy(_raw)


def strerror(code):
    return lib.pn2_strerror(int(code)).decode()


def check(code, what):
    if code != 0:
        raise Pn2Error("%s failed: %s (code %d)" % (what, strerror(code), code))


def ptr(t, byte_offset=0):
    """device pointer of a tensor (None -> NULL), optionally `byte_offset` bytes into it."""
    return None if t is None else c_void_p(t.data_ptr() + byte_offset)


def rows_in_place(t):
    """(tensor, ld) for a (b, n, c) float32 tensor the *_ld entry points can read where it lies: rows `ld` floats apart, clouds
    n * ld floats apart -- a dense tensor (ld = c) or a column block of a wider dense one (point_cloud[:, :, 0:3] of a (b,n,6)
    batch: ld = 6).  Anything else -- other layouts, other dtypes (ld counts FLOATS) -- is copied dense: ld = c elements."""
    t = t.detach()
    if t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) >= t.shape[2] and t.stride(0) == t.shape[1] * t.stride(1) \
            and t.data_ptr() % 4 == 0:
        return t, int(t.stride(1))
    t = t.contiguous()
    return t, int(t.shape[2])


def stream_ptr():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(name, where, *args, may_refuse=False, stream=True):
    """Call entry point `name` with `args` + torch's current stream (stream=False: a host-side query that takes none), on the
    device of `where` (a tensor or a device).  The entry point is looked up on `lib` at call time (the trace / dup hooks see it).
    -> True; with may_refuse, False when the library reports the configuration as unsupported (PN2_EUNSUP).  Every other failure
    raises Pn2Error naming the entry point."""
    with torch.cuda.device(getattr(where, "device", where)):
        rc = getattr(lib, name)(*args, stream_ptr()) if stream else getattr(lib, name)(*args)
    if may_refuse and rc == PN2_EUNSUP:
        return False
    check(rc, name)
    return True


def aligned(nbytes, device):
    """a uint8 device buffer of nbytes whose first byte is 256-aligned (what every workspace argument asks for; the text kernels
    load 16 bytes at a time)"""
    raw = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    off = (-raw.data_ptr()) % 256
    return raw[off:off + nbytes]


def workspace(query, dev, *size_args):
    """the workspace of one call: the size query `query` (..., &bytes) is asked with `size_args` and a 256-aligned uint8 view of
    that many bytes on `dev` comes back, to be passed as ptr(ws), ws.numel()"""
    need = u64_array([0])  # written by the query
    launch(query, dev, *size_args, need, stream=False)
    return aligned(int(need[0]), dev)


def nbytes(t):
    return t.numel() * t.element_size()


# Host arrays for the entry points that read widths[] / pointer tables: ctypes arrays, accepted as they are where the argtype is
# c_void_p.  The caller holds them until the call has returned (the library reads them before it returns).
def int_array(values):
    return (c_int * len(values))(*[int(v) for v in values])


def float_array(values):
    return (c_float * len(values))(*[float(v) for v in values])


def u64_array(values):
    """64-bit unsigned: byte counts and offsets (size_t), raw 64-bit payloads"""
    return (ctypes.c_uint64 * len(values))(*[int(v) for v in values])


def ptr_table(tensors):
    """host table of device pointers (None -> NULL)"""
    return (c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def layer_arrays(ws, bs):
    """-> nlayers, widths[], weight pointers, bias pointers of a stack of dense layers (ws[i]: (cin_i, cout_i))"""
    return len(ws), int_array([w.shape[1] for w in ws]), ptr_table(ws), ptr_table(bs)


def require_cuda(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("pn2 ops run on the MI355X only: got a %s tensor (there is no CPU path in the "
                             "product; the CPU oracle lives under oracle/ for tests)" % t.device)
