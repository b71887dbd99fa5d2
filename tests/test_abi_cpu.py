"""CPU tests of the drop-in boundary: the C-ABI library loads without a GPU, exports every
symbol include/pn2_abi.h declares, and validates arguments before touching the device."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    """include/pn2_abi.h through the package's own parser (the one parser in the tree), from this file's idea of the path"""
    from pn2_amd import _abi
    return _abi.load(os.path.join(ROOT, "include", "pn2_abi.h"))


def _declared():
    return sorted(_header().functions)


def test_header_declares_the_nine_reference_ops():
    names = _declared()
    for n in ["pn2_farthest_point_sample", "pn2_gather_point", "pn2_gather_point_grad", "pn2_query_ball_point",
              "pn2_group_point", "pn2_group_point_grad", "pn2_three_nn", "pn2_three_interpolate",
              "pn2_three_interpolate_grad", "pn2_sa_mlp_max_fused", "pn2_linear", "pn2_fp_interp_concat"]:
        assert n in names


def test_library_exports_every_declared_symbol(pn2):
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for n in _declared():
        assert hasattr(lib, n), n
    assert pn2._lib.lib.pn2_abi_version() == 2
    assert b"gfx950" in pn2._lib.lib.pn2_build_info()
    # the shipped library has no tuning hooks: no process-global kernel-selection state behind the ABI
    assert not hasattr(lib, "pn2_debug_set") and not hasattr(lib, "pn2_debug_set_grouping")


def test_bn_workspace_states_match_the_header(pn2):
    """PN2_BN_WS_* of include/pn2_abi.h are 0..3 in the documented order and _lib.BN_WS_* are the same numbers"""
    states = {k[len("PN2_BN_WS_"):]: v for k, v in _header().constants.items() if k.startswith("PN2_BN_WS_")}
    assert states == {"UNCLEARED": 0, "ZEROED": 1, "SUMMED": 2, "FOLDED": 3}
    assert list(states) == ["UNCLEARED", "ZEROED", "SUMMED", "FOLDED"]
    for name, value in states.items():
        assert getattr(pn2._lib, "BN_WS_" + name) == value, name


# forward / backward x the suffixes for a caller-zeroed workspace and for one that already holds the sums
REMOVED_BN_ALIASES = ["pn2_bn_relu_%s_%s" % (d, sfx) for d in ("forward", "backward") for sfx in ("ws" + "0", "stats")]


def test_bn_alias_entry_points_are_gone(pn2):
    """ABI version 2 dropped the entry points that only passed a constant state to the _mode forms"""
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for n in REMOVED_BN_ALIASES:
        assert not hasattr(lib, n), n
        assert n not in pn2._lib.SIGNATURES and n not in _declared(), n


def test_bn_state_range_is_checked_before_the_pointers(pn2):
    """a stats_mode outside PN2_BN_WS_UNCLEARED .. PN2_BN_WS_FOLDED is PN2_EINVAL even when every pointer is NULL (PN2_ENULL
    otherwise): the range check comes first"""
    L, nul = pn2._lib.lib, None
    for mode in (-1, 4):
        assert L.pn2_bn_relu_forward_mode(64, 32, nul, nul, nul, nul, 1e-3, 0.9, 1, nul, nul, nul, 0, mode, nul, nul, nul, nul) == -1
        assert L.pn2_bn_relu_forward_pool(64, 32, nul, nul, nul, nul, 1e-3, 0.9, 1, 32, nul, nul, nul, 0, mode, nul, nul, nul, nul,
                                          nul, nul) == -1
        assert L.pn2_bn_relu_backward_mode(64, 32, nul, nul, nul, nul, nul, nul, 1, 0, nul, nul, nul, 0, mode, nul, nul, nul, nul) == -1
    for mode in range(4):  # a known state reaches the pointer checks
        assert L.pn2_bn_relu_forward_mode(64, 32, nul, nul, nul, nul, 1e-3, 0.9, 1, nul, nul, nul, 0, mode, nul, nul, nul, nul) == -2
        assert L.pn2_bn_relu_backward_mode(64, 32, nul, nul, nul, nul, nul, nul, 1, 0, nul, nul, nul, 0, mode, nul, nul, nul, nul) == -2


def test_python_signatures_cover_the_header(pn2):
    decl = set(_declared()) - {"pn2_abi_version", "pn2_build_info", "pn2_strerror",
                               "pn2_interpolate_label_workspace_bytes", "pn2_fps_large_workspace_bytes",
                               "pn2_bn_workspace_bytes", "pn2_three_interpolate_grad_workspace_bytes",
                               "pn2_group_point_grad_workspace_bytes", "pn2_voxel_downsample_workspace_bytes",
                               "pn2_scatter_plan_bytes", "pn2_ball_query_bin_bytes"}  # bound separately: size_t
    assert decl <= set(pn2._lib.SIGNATURES)
    # ... and nothing is bound that the header does not declare (no undocumented entry points in the product)
    assert set(pn2._lib.SIGNATURES) <= decl
    assert pn2._lib.lib.pn2_interpolate_label_workspace_bytes(1000) > 2 * (1 << 21) * 4  # two cell tables + lists


def test_trace_table_positions_match_the_signatures(pn2):
    """_lib._TRACE_ARGS tells the benchmark trace where an entry point keeps nlayers and the host widths[] array, and which dense
    entry point an in-place (*_ld) form is recorded as: every position is checked against the bound signature."""
    L = pn2._lib
    assert L._TRACE_ARGS
    for name, (nl_at, w_at, dense, drop) in L._TRACE_ARGS.items():
        sig = L.SIGNATURES[name]  # KeyError: the table names an entry point that is not bound
        assert (nl_at is None) == (w_at is None), name
        if w_at is not None:
            assert sig[nl_at] is ctypes.c_int, name
            assert sig[w_at] is ctypes.c_void_p, name
        numeric = [i for i, t in enumerate(sig) if t is not ctypes.c_void_p]
        if name.endswith("_ld"):
            assert dense in L.SIGNATURES and dense == name[:-3], name
            assert drop, name
            # dropping the strides leaves the dense form's numeric arguments, type by type
            kept = [sig[i] for k, i in enumerate(numeric) if k not in drop]
            assert kept == [t for t in L.SIGNATURES[dense] if t is not ctypes.c_void_p], name
            for k in drop:
                assert sig[numeric[k]] is ctypes.c_int, name
        else:
            assert dense is None and drop == (), name
    # every *_ld entry point is in the table: none is recorded under its own name
    assert {n for n in L.SIGNATURES if n.endswith("_ld")} <= set(L._TRACE_ARGS)
    # the size_t queries are bound from the header: name -> number of int arguments
    queries = {"pn2_fps_large_workspace_bytes": 2, "pn2_ball_query_bin_bytes": 1, "pn2_interpolate_label_workspace_bytes": 1,
               "pn2_three_interpolate_grad_workspace_bytes": 3, "pn2_scatter_plan_bytes": 3,
               "pn2_group_point_grad_workspace_bytes": 4, "pn2_voxel_downsample_workspace_bytes": 1, "pn2_bn_workspace_bytes": 1}
    assert {name for name, f in _header().functions.items() if f.restype is ctypes.c_size_t} == set(queries)
    for name, nargs in queries.items():
        fn = getattr(L._raw, name)
        assert fn.restype is ctypes.c_size_t and fn.argtypes == [ctypes.c_int] * nargs, name


def test_every_traced_parameter_name_is_in_the_trace_table(pn2):
    """a prototype with a parameter named nlayers, widths or ld* is decoded by the benchmark trace"""
    for name, f in _header().functions.items():
        if any(a in ("nlayers", "widths") or a.startswith("ld") for a in f.argnames):
            assert name in pn2._lib._TRACE_ARGS, name


def test_stateful_set_names_bound_entry_points(pn2):
    L = pn2._lib
    assert L._STATEFUL <= set(L.SIGNATURES)
    for name, f in _header().functions.items():  # a moving average is caller state: never launched twice by the dup hook
        if "running_mean" in f.argnames:
            assert name in L._STATEFUL, name


def test_six_signatures_by_hand(pn2):
    """one entry point per kind of scalar the header uses, written out by hand against the derived table"""
    i, f, d, p, z, ll = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong
    S = pn2._lib.SIGNATURES
    assert S["pn2_farthest_point_sample"] == [i, i, i, p, p, p, i, p]
    assert S["pn2_fps_large"] == [i, i, i, p, p, z, p, p, i, p]
    assert S["pn2_bn_relu_forward_mode"] == [ll, i, p, p, p, p, f, f, i, p, p, p, z, i, p, p, p, p]
    assert S["pn2_scene_extract_z_box"] == [i, p, i, p, d, d, d, i, p, p, p]
    assert S["pn2_dataset_sample"] == [i] * 6 + [p] * 7 + [i, d, d, ctypes.c_ulonglong, p, p, p, p, i, p, p, z] + [p] * 7
    assert "pn2_fps_large_workspace_bytes" not in S
    for name, sig in S.items():
        fn = getattr(pn2._lib._raw, name)
        assert fn.argtypes == sig and fn.restype is i, name
    q = pn2._lib._raw.pn2_fps_large_workspace_bytes
    assert q.restype is z and q.argtypes == [i, i]
    assert pn2._lib._raw.pn2_build_info.restype is ctypes.c_char_p and pn2._lib._raw.pn2_strerror.argtypes == [i]


MINI_HEADER = """
/* a block comment that mentions pn2_x(int a); and spans
 * lines */
#ifndef MINI_H_
#define MINI_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PN2_ABI_VERSION 7
#define PN2_EBAD (-3)  /* parenthesised */
enum { PN2_A = 0, PN2_B = 1, PN2_C = (-2) };
int pn2_none(void);
const char *pn2_name(int code);
size_t pn2_bytes(int b, int n);
int pn2_many(const float *inp, int *const *table, float* const* x, size_t nbytes, long long rows,
             unsigned long long seed, double half_x,
             const int ld1, float eps, void *stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_an_inline_header():
    from pn2_amd import _abi
    i, p = ctypes.c_int, ctypes.c_void_p
    abi = _abi.parse(MINI_HEADER)
    assert list(abi.functions) == ["pn2_none", "pn2_name", "pn2_bytes", "pn2_many"]  # pn2_x lives in a comment
    assert abi.functions["pn2_none"] == (i, [], ())
    assert abi.functions["pn2_name"] == (ctypes.c_char_p, [i], ("code",))
    assert abi.functions["pn2_bytes"] == (ctypes.c_size_t, [i, i], ("b", "n"))
    many = abi.functions["pn2_many"]
    assert many.restype is i
    assert many.argtypes == [p, p, p, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_double, i, ctypes.c_float, p]
    assert many.argnames == ("inp", "table", "x", "nbytes", "rows", "seed", "half_x", "ld1", "eps", "stream")
    assert abi.constants == {"PN2_ABI_VERSION": 7, "PN2_EBAD": -3, "PN2_A": 0, "PN2_B": 1, "PN2_C": -2}


@pytest.mark.parametrize("proto, message", [
    ("int pn2_bad(short n);", "pn2_bad"),                        # unknown scalar: never bound as int
    ("int pn2_bad(unsigned n);", "pn2_bad"),
    ("int pn2_bad(int);", "pn2_bad"),                            # no parameter name
    ("int pn2_bad(int widths[4]);", "array or function-pointer"),
    ("int pn2_bad(int (*cb)(int, int), void *stream);", "array or function-pointer"),
    ("void pn2_bad(int n);", "pn2_bad"),                         # unknown return type
    ("int pn2_bad(int n)", "pn2_bad"),                           # no `;`: cannot be split
    ("int pn2_bad int n;", "pn2_bad"),
    ("int pn2_none(int a);", "declared twice"),
    ("#define PN2_HALF 0.5", "PN2_HALF"),
    ("enum { PN2_A = 0, PN2_NEXT };", "PN2_NEXT"),             # an implicit value is not guessed
])
def test_parser_refuses_what_it_does_not_understand(proto, message):
    from pn2_amd import _abi
    with pytest.raises(ValueError, match=message.replace("(", r"\(")):
        _abi.parse("int pn2_none(void);\n" + proto + "\n")


def test_parser_says_where_it_looked_for_a_missing_header(tmp_path):
    from pn2_amd import _abi
    missing = str(tmp_path / "include" / "pn2_abi.h")
    with pytest.raises(ImportError, match=missing):
        _abi.load(missing)


def test_header_path_is_shared_with_the_build(pn2):
    assert os.path.samefile(pn2.build.HEADER, os.path.join(ROOT, "include", "pn2_abi.h"))
    assert pn2._lib.ABI.constants["PN2_ABI_VERSION"] == 2 and pn2._lib.ABI.constants["PN2_FPS_MAX_REG_POINTS"] == 16384
    assert (pn2._lib.PN2_EUNSUP, pn2._lib.ABI.constants["PN2_ARITH_FMA_ALT"]) == (-4, 2)


def test_launch_helper_host_arrays(pn2):
    L = pn2._lib
    a = L.int_array([3, 4.0, True])
    assert list(a) == [3, 4, 1] and isinstance(a, ctypes.Array)
    assert list(L.float_array([1, 0.5])) == [1.0, 0.5]
    assert list(L.u64_array([0, 2 ** 64 - 1])) == [0, 2 ** 64 - 1]
    t = L.ptr_table([None])
    assert len(t) == 1 and t[0] is None
    # accepted as they are where the argtype is c_void_p
    assert ctypes.c_void_p.from_param(a) is not None and ctypes.c_void_p.from_param(t) is not None
    assert L.ptr(None) is None


def test_argument_validation_needs_no_gpu(pn2):
    L = pn2._lib.lib
    nul = None
    assert L.pn2_farthest_point_sample(0, 8, 4, nul, nul, nul, 1, nul) == -1      # PN2_EINVAL
    assert L.pn2_farthest_point_sample(1, 8, 4, nul, nul, nul, 1, nul) == -2      # PN2_ENULL
    assert L.pn2_query_ball_point(1, 8, 4, 0.0, 4, nul, nul, nul, nul, 1, nul) == -1  # radius must be > 0
    assert L.pn2_query_ball_point(1, 8, 4, 0.5, 0, nul, nul, nul, nul, 1, nul) == -1  # nsample must be > 0
    assert L.pn2_three_nn(1, 8, 2, nul, nul, nul, nul, nul) == -1                  # needs >= 3 known points
    assert L.pn2_group_point(1, 8, 0, 4, 4, nul, nul, nul, nul) == -1
    assert b"PN2_ENULL" in L.pn2_strerror(-2)
    assert L.pn2_interpolate_label_with_color(10, 10, nul, nul, nul, nul, nul, 0, nul, 0, nul) == -1   # knn > 0
    assert L.pn2_interpolate_label_with_color(10, 10, nul, nul, nul, nul, nul, 3, nul, 0, nul) == -2
    assert L.pn2_fp_mlp_fused(1, 8, 4, 0, 8, nul, nul, nul, nul, 1, nul, nul, nul, nul, nul) == -2
    assert L.pn2_mlp_chain(0, 8, nul, 1, nul, nul, nul, 0, nul, nul) == -1
    assert L.pn2_scene_extract_z_box(0, nul, 1, nul, 5.0, 5.0, 1.0, 8, nul, nul, nul) == -1
    assert L.pn2_scene_extract_z_box(10, nul, 1, nul, 5.0, 5.0, 1.0, 8, nul, nul, nul) == -2
    assert L.pn2_scene_sample(1, 0, 8, nul, nul, nul, nul, nul, nul, 5.0, 5.0, nul, nul, nul, nul, nul, nul, nul) == -1
    assert L.pn2_voxel_downsample(10, nul, nul, nul, 0.0, nul, nul, nul, nul, nul, nul, 0, nul) == -1   # voxel_size > 0
    assert L.pn2_voxel_downsample(10, nul, nul, nul, 0.05, nul, nul, nul, nul, nul, nul, 0, nul) == -2
    # pn2_coarse_geometry: host arrays of per-level sizes and of device pointers
    import ctypes
    one_i = lambda v: (ctypes.c_int * 1)(v)        # noqa: E731
    one_f = lambda v: (ctypes.c_float * 1)(v)      # noqa: E731
    one_p = lambda v: (ctypes.c_void_p * 1)(v)     # noqa: E731
    fake = ctypes.c_void_p(4096)                   # never dereferenced: every call below is refused before a launch
    assert L.pn2_coarse_geometry(1, 64, 1, nul, nul, nul, nul, nul, nul, nul, nul, nul, nul, nul, nul, 2, 1, nul) == -2
    args = lambda b, n0, m, nn: (b, n0, 1, one_i(m), one_f(0.5), one_i(8), fake, nul, one_p(4096), one_p(4096), one_p(4096), nul,   # noqa: E731
                                 one_p(4096) if nn else nul, one_p(4096) if nn else nul, nul, 2, 1, nul)
    assert L.pn2_coarse_geometry(*args(0, 64, 16, False)) == -1       # b > 0
    assert L.pn2_coarse_geometry(*args(1, 2048, 16, False)) == -4     # PN2_EUNSUP: source cloud above 1024 points
    assert L.pn2_coarse_geometry(*args(1, 64, 65, False)) == -4       # more samples than points
    assert L.pn2_coarse_geometry(*args(1, 1024, 512, True)) == -4     # 3-NN table over more than 256 samples
    assert L.pn2_coarse_geometry(*args(1, 64, 2, True)) == -1         # 3-NN needs >= 3 known points
    a = list(args(1, 64, 16, False)); a[-3] = 7
    assert L.pn2_coarse_geometry(*a) == -1                            # unknown arithmetic mode
    # r05: the *_ld entry points (row stride in floats) and pn2_relu_grad: refused before any launch
    assert L.pn2_fps_nested_ld(1, 64, 8, fake, 2, fake, nul, nul, nul, 2, nul) == -1             # ld >= 3
    assert L.pn2_fps_nested_ld(1, 64, 8, nul, 6, fake, nul, nul, nul, 2, nul) == -2              # inp
    assert L.pn2_fps_nested_ld(1, 20000, 8, fake, 6, fake, nul, nul, nul, 2, nul) == -4          # streaming kernel: dense rows only
    assert L.pn2_fps_nested_ld(1, 64, 8, fake, 6, fake, nul, nul, nul, 9, nul) == -1             # arithmetic mode
    assert L.pn2_query_ball_point_ld(1, 8192, 1024, 0.5, 32, fake, 2, fake, fake, fake, 1, nul) == -1
    assert L.pn2_query_ball_point_ld(1, 8192, 1024, -1.0, 32, fake, 6, fake, fake, fake, 1, nul) == -1
    assert L.pn2_query_ball_point_ld(1, 8192, 1024, 0.5, 32, fake, 6, nul, fake, fake, 1, nul) == -2
    assert L.pn2_query_ball_point_ld(1, 1000, 100, 0.5, 32, fake, 6, fake, fake, fake, 1, nul) == -4   # outside the LDS-grid kernel
    assert L.pn2_three_nn_ld(1, 64, 2, fake, 6, fake, fake, fake, nul) == -1                     # >= 3 known points
    assert L.pn2_ball_query_bin_ld(1, 8192, 0.5, fake, 2, fake, 1 << 20, nul) == -1              # r06: ld >= 3
    assert L.pn2_ball_query_bin_ld(1, 8192, 0.5, nul, 6, fake, 1 << 20, nul) == -2
    assert L.pn2_ball_query_bin_ld(1, 20000, 0.5, fake, 6, fake, 1 << 20, nul) == -4             # outside the LDS-grid kernel
    assert L.pn2_three_nn_ld(1, 64, 16, fake, 1, fake, fake, fake, nul) == -1                    # ld >= 3
    assert L.pn2_three_nn_ld(1, 64, 16, fake, 6, nul, fake, fake, nul) == -2
    w1 = one_i(32)
    assert L.pn2_sa_mlp_max_fused_ld(1, 64, 8, 32, 3, fake, 2, fake, fake, 6, fake, 1, w1, one_p(4096), one_p(4096), fake, nul) == -1
    assert L.pn2_sa_mlp_max_fused_ld(1, 64, 8, 32, 3, fake, 6, fake, fake, 2, fake, 1, w1, one_p(4096), one_p(4096), fake, nul) == -1
    assert L.pn2_sa_mlp_max_fused_ld(1, 64, 8, 32, 8, fake, 6, fake, fake, 16, fake, 1, w1, one_p(4096), one_p(4096), fake, nul) == -4  # 16-byte gathers: dense rows
    assert L.pn2_fp_mlp_fused_pre_ld(1, 64, 16, 3, fake, fake, fake, 2, fake, 2, w1, one_p(4096), one_p(4096), fake, nul) == -1    # ld < c1
    assert L.pn2_relu_grad(0, fake, fake, fake, nul) == -1
    assert L.pn2_relu_grad(16, nul, fake, fake, nul) == -2


# ---- refusals of the fused-MLP entry points (csrc/pn2_sa_fused.hip, pn2_sa_fused_bf16.hip, pn2_mlp_wide.hip) -------------------
# One reader (csrc/pn2_layer_stack.h) validates nlayers / widths[] / w[] / bias[] for all fifteen; what a refused call returns,
# and which fault wins where two are present, is part of the ABI.  REFUSAL_TABLE was printed by `python tests/test_abi_cpu.py`
# on the commit before the shared reader: one row per fault, one column per entry point of REFUSAL_ENTRIES.
#   I = PN2_EINVAL, N = PN2_ENULL, R = PN2_ERANGE, U = PN2_EUNSUP;  . = not called: the entry point has no such argument, or it
#   accepts the combination (a misaligned bias on the chains, a NULL w[0] with c1 == 0) and would go on to launch.
# A fault is a list of changes to a call that would be accepted, joined by " + ":
#   nlayers=0 / nlayers=max+1      widths=NULL / w=NULL / bias=NULL (the host tables)
#   widths[0]=48, widths[last]=0   a width at the first / last layer
#   w[0]=NULL, bias[last]=NULL     a device pointer of a layer;  =odd: 4 bytes past a 16-byte boundary
#   c1=0, pool=7                   a scalar argument of that name
#   range                          the row count pushed past what an int holds (b = m = n = 2^20; rows = 2^31 - 8)
# Device pointers are placeholders that are never dereferenced; the host arrays are real.  Every call of pn2_sa_mlp_max_fused*
# keeps nsample = 32, so no zero-fill is queued even on the commit that queued it ahead of the kernel choice.
REFUSAL_CODES = {"I": -1, "N": -2, "R": -3, "U": -4}
_CHAIN3, _CHAIN2, _CHAIN128, _WIDE = [64, 64, 128], [128, 128], [128, 128, 128], [128, 256, 512]
REFUSAL_ENTRIES = [  # entry point, widths of a call it accepts (its most layers), scalar arguments that differ from _SCALARS
    ("pn2_sa_mlp_max_fused", _CHAIN3, {}), ("pn2_sa_mlp_max_fused_ld", _CHAIN3, {}), ("pn2_sa_mlp_rows_fused", _CHAIN2, {}),
    ("pn2_sa_mlp_fused_pre", _CHAIN3, {"pool": 1}), ("pn2_sa_mlp_max_fused_bf16", _CHAIN3, {}), ("pn2_mlp_chain", _CHAIN2, {}),
    ("pn2_fp_mlp_fused", _CHAIN2, {}), ("pn2_fp_mlp_fused_pre", _CHAIN128, {}), ("pn2_fp_mlp_fused_pre_ld", _CHAIN128, {}),
    ("pn2_fp_mlp_fused_pre_schedule", _CHAIN128, {}), ("pn2_mlp_wide", _WIDE, {}), ("pn2_sa_mlp_wide", _WIDE, {"pool": 1}),
    ("pn2_fp_mlp_wide", _WIDE, {}), ("pn2_fp_mlp_wide_pre", _WIDE, {}), ("pn2_sa_mlp_wide_pre", _WIDE, {"pool": 1})]
_SCALARS = dict(b=1, n=64, m=8, nsample=32, c=16, c1=4, c2=8, rows=64, cin=8, x_stride=8, relu_last=1, pool=0, schedule=0,
                ld_xyz=3, ld_points=16, ld_points1=4)
_RANGE = dict(b=1 << 20, n=1 << 20, m=1 << 20, rows=(1 << 31) - 8)
REFUSAL_FAULTS = [
    "nlayers=0", "nlayers=max+1", "widths=NULL", "w=NULL", "bias=NULL",
    "widths[0]=0", "widths[0]=48", "widths[0]=160", "widths[0]=64", "widths[0]=384",
    "widths[last]=0", "widths[last]=48", "widths[last]=160", "widths[last]=64", "widths[last]=384",
    "w[0]=NULL", "w[last]=NULL", "bias[0]=NULL", "bias[last]=NULL",
    "w[0]=odd", "w[last]=odd", "bias[0]=odd", "bias[last]=odd",
    "c1=0 + w[0]=NULL", "c1=0 + w[0]=NULL + w[last]=NULL", "c1=0 + w[0]=NULL + bias[0]=NULL", "c1=0 + w[0]=odd",
    "range", "pool=7",
    # two faults at once: the precedence
    "nlayers=0 + widths=NULL", "nlayers=max+1 + w=NULL", "nlayers=max+1 + widths[0]=48", "nlayers=max+1 + widths[0]=64",
    "nlayers=max+1 + range", "widths=NULL + range",
    "widths[0]=48 + w[0]=NULL", "widths[0]=64 + w[0]=NULL", "w[0]=odd + bias[0]=NULL", "bias[0]=odd + w[0]=NULL",
    "widths[last]=0 + bias[0]=NULL", "w[0]=NULL + w[last]=odd", "w[0]=odd + bias[last]=NULL", "bias[last]=odd + w[last]=NULL",
    "widths[0]=48 + range", "widths[0]=64 + range", "w[last]=NULL + range", "w[last]=odd + range",
    "pool=7 + w[0]=NULL", "pool=7 + widths[last]=64", "pool=7 + range",
]
REFUSAL_TABLE = [
    ("nlayers=0",                                 "I I I I I I I I I I U U U U U"),
    ("nlayers=max+1",                             "U U U U U U U U U U U U U U U"),
    ("widths=NULL",                               "N N N N N N N N N N N N N N N"),
    ("w=NULL",                                    "N N N N N N N N N N N N N N N"),
    ("bias=NULL",                                 "N N N N N N N N N N N N N N N"),
    ("widths[0]=0",                               "U U U U U U U U U U U U U U U"),
    ("widths[0]=48",                              "U U U U U U U U U U U U U U U"),
    ("widths[0]=160",                             "U U U U U U U U U U U U U U U"),
    ("widths[0]=64",                              ". . U . . . . U U U U U U U U"),
    ("widths[0]=384",                             "U U U U U U U U U U U U U U U"),
    ("widths[last]=0",                            "U U U U U U U U U U U U U U U"),
    ("widths[last]=48",                           "U U U U U U U U U U U U U U U"),
    ("widths[last]=160",                          "U U U U U U U U U U U U U U U"),
    ("widths[last]=64",                           ". . U U U U U U U U U U U U U"),
    ("widths[last]=384",                          "U U U U U U U U U U U U U U U"),
    ("w[0]=NULL",                                 "N N N N N N N N N N N N N N N"),
    ("w[last]=NULL",                              "N N N N N N N N N N N N N N N"),
    ("bias[0]=NULL",                              "N N N N N N N N N N N N N N N"),
    ("bias[last]=NULL",                           "N N N N N N N N N N N N N N N"),
    ("w[0]=odd",                                  "U U U U . U U U U U U U U U U"),
    ("w[last]=odd",                               "U U U U . U U U U U U U U U U"),
    ("bias[0]=odd",                               ". . . . . . . . . . U U U U U"),
    ("bias[last]=odd",                            ". . . . . . . . . . U U U U U"),
    ("c1=0 + w[0]=NULL",                          ". . . . . . N . . . . . N I ."),
    ("c1=0 + w[0]=NULL + w[last]=NULL",           ". . . . . . N N N N . . N I ."),
    ("c1=0 + w[0]=NULL + bias[0]=NULL",           ". . . . . . N N N N . . N I ."),
    ("c1=0 + w[0]=odd",                           ". . . . . . U U U U . . U I ."),
    ("range",                                     "R R R R R . R R R R R R R R R"),
    ("pool=7",                                    ". . . . . U . . . . U . . . ."),
    ("nlayers=0 + widths=NULL",                   "I I I I I I I I I I U U U U U"),
    ("nlayers=max+1 + w=NULL",                    "N N N N N N N N N N U U U U U"),
    ("nlayers=max+1 + widths[0]=48",              "U U U U U U U U U U U U U U U"),
    ("nlayers=max+1 + widths[0]=64",              "U U U U U U U U U U U U U U U"),
    ("nlayers=max+1 + range",                     "U U R U U U R R R R U U U U U"),
    ("widths=NULL + range",                       "N N N N N N N N N N N N N N N"),
    ("widths[0]=48 + w[0]=NULL",                  "U U U U U U U N N N U U U U U"),
    ("widths[0]=64 + w[0]=NULL",                  "N N N N N N N N N N U U U U U"),
    ("w[0]=odd + bias[0]=NULL",                   "N N N N N N N N N N N N N N N"),
    ("bias[0]=odd + w[0]=NULL",                   "N N N N N N N N N N N N N N N"),
    ("widths[last]=0 + bias[0]=NULL",             "N N N N N N N N N N N N N N N"),
    ("w[0]=NULL + w[last]=odd",                   "N N N N N N N N N N N N N N N"),
    ("w[0]=odd + bias[last]=NULL",                "U U U U N U U U U U U U U U U"),
    ("bias[last]=odd + w[last]=NULL",             "N N N N N N N N N N N N N N N"),
    ("widths[0]=48 + range",                      "R R R R R U R R R R U U U U U"),
    ("widths[0]=64 + range",                      "R R R R R . R R R R U U U U U"),
    ("w[last]=NULL + range",                      "R R R R R N R R R R N N N N N"),
    ("w[last]=odd + range",                       "R R R R R U R R R R U U U U U"),
    ("pool=7 + w[0]=NULL",                        ". . . N . U . . . . N N . . N"),
    ("pool=7 + widths[last]=64",                  ". . . U . U . . . . U U . . U"),
    ("pool=7 + range",                            ". . . R . U . . . . U R . . R"),
]


def _refusal_call(pn2, entry, widths, own, fault):
    """-> the code `entry` returns for an acceptable call with `fault` applied, or None when the entry point lacks an argument
    the fault names"""
    f = _header().functions[entry]
    nmax = len(widths)
    scal = dict(_SCALARS, **own)
    lay = dict(nlayers=nmax, widths=list(widths) + [128], w=[4096] * (nmax + 1), bias=[8192] * (nmax + 1))
    tables = dict(widths=True, w=True, bias=True)
    for atom in fault.split(" + "):
        if atom == "range":
            scal.update(_RANGE)
            continue
        key, value = atom.split("=", 1)
        if "[" in key:
            name, at = key[:-1].split("[")
            at = 0 if at == "0" else nmax - 1
            if name == "widths":
                lay[name][at] = int(value)
            elif value == "NULL":
                lay[name][at] = None
            else:  # odd
                lay[name][at] += 4
        elif value == "NULL":
            tables[key] = False
        elif key == "nlayers":
            lay["nlayers"] = nmax + 1 if value == "max+1" else int(value)
        else:
            if key not in f.argnames:
                return None
            scal[key] = int(value)
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call of the table is refused before a launch
    host = dict(widths=(ctypes.c_int * (nmax + 1))(*lay["widths"]), w=(ctypes.c_void_p * (nmax + 1))(*lay["w"]),
                bias=(ctypes.c_void_p * (nmax + 1))(*lay["bias"]))
    args = []
    for name, t in zip(f.argnames, f.argtypes):
        if name == "nlayers":
            args.append(lay["nlayers"])
        elif name in host:
            args.append(host[name] if tables[name] else None)
        elif name == "stream":
            args.append(None)
        elif t is ctypes.c_void_p:
            args.append(fake)
        else:
            args.append(scal[name])
    return getattr(pn2._lib.lib, entry)(*args)


def test_refusal_table_is_well_formed():
    assert len(REFUSAL_ENTRIES) == 15 and len({e[0] for e in REFUSAL_ENTRIES}) == 15
    assert [f for f, _ in REFUSAL_TABLE] == REFUSAL_FAULTS
    for fault, cells in REFUSAL_TABLE:
        assert len(cells.split()) == 15 and set(cells.split()) <= set(REFUSAL_CODES) | {"."}, fault
    for col, (entry, _, _) in enumerate(REFUSAL_ENTRIES):  # every entry point is refused for each kind of fault the issue names
        rows = {f for f, cells in REFUSAL_TABLE if cells.split()[col] != "."}
        assert {"nlayers=0", "nlayers=max+1", "widths=NULL", "w=NULL", "bias=NULL", "widths[0]=0", "w[last]=NULL", "bias[0]=NULL",
                "bias[last]=NULL", "widths[0]=48 + w[0]=NULL", "w[0]=odd + bias[0]=NULL"} <= rows, entry


@pytest.mark.parametrize("col", range(15), ids=[e[0] for e in REFUSAL_ENTRIES])
def test_fused_mlp_refusals_are_unchanged(pn2, col):
    """every refused layer stack returns what the commit before the shared reader returned, precedence included"""
    entry, widths, own = REFUSAL_ENTRIES[col]
    called = 0
    for fault, cells in REFUSAL_TABLE:
        cell = cells.split()[col]
        if cell == ".":
            continue
        rc = _refusal_call(pn2, entry, widths, own, fault)
        assert rc in REFUSAL_CODES.values(), (entry, fault, rc)
        assert rc == REFUSAL_CODES[cell], (entry, fault, rc)
        called += 1
    assert called >= 25, entry


def test_rows_in_place_recognises_column_blocks():
    """_lib.rows_in_place: a dense (b,n,c) tensor or a column block of a wider dense one is read where it lies (row stride in
    floats); anything else is copied.  Host logic only."""
    import torch
    from pn2_amd._lib import rows_in_place
    pc = torch.arange(2 * 5 * 6, dtype=torch.float32).reshape(2, 5, 6)
    t, ld = rows_in_place(pc[:, :, 0:3])
    assert ld == 6 and t.data_ptr() == pc.data_ptr() and not t.is_contiguous()
    t, ld = rows_in_place(pc[:, :, 3:6])
    assert ld == 6 and t.data_ptr() == pc.data_ptr() + 12
    t, ld = rows_in_place(pc)
    assert ld == 6 and t.data_ptr() == pc.data_ptr()
    t, ld = rows_in_place(pc[:, ::2, 0:3])          # every second row: clouds are no longer n * ld apart
    assert ld == 3 and t.is_contiguous() and torch.equal(t, pc[:, ::2, 0:3])
    t, ld = rows_in_place(pc.transpose(1, 2))        # not row-major at all
    assert ld == 5 and t.is_contiguous()
    t, ld = rows_in_place(pc[:1, :, 0:3])            # a single cloud
    assert torch.equal(t, pc[:1, :, 0:3]) and ld in (3, 6)


def test_ops_refuse_cpu_tensors_loudly(pn2):
    import torch
    x = torch.zeros(1, 16, 3)
    with pytest.raises(ValueError, match="MI355X only"):
        pn2.farthest_point_sample(4, x)
    with pytest.raises(ValueError, match="MI355X only"):
        pn2.three_nn(x, x)
    with pytest.raises(ValueError, match="positive npoint"):
        pn2.farthest_point_sample(0, x)
    with pytest.raises(ValueError, match="positive radius"):
        pn2.query_ball_point(-1.0, 4, x, x)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "pn2_oracle" not in txt, f


if __name__ == "__main__":  # prints REFUSAL_TABLE's rows from the library in the tree (see the comment above the table)
    import sys
    sys.path.insert(0, ROOT)
    import pn2_amd
    letter = {v: k for k, v in REFUSAL_CODES.items()}
    for fault in REFUSAL_FAULTS:
        cells = [letter.get(_refusal_call(pn2_amd, e, wd, own, fault), ".") for e, wd, own in REFUSAL_ENTRIES]
        print("    (%-44s %r)," % ('"%s",' % fault, " ".join(cells)))
