"""CPU tests of the two multi-scale entry points behind the training path of pointnet_sa_module_msg (pn2_sa_hoist_rows_multi_bn,
pn2_scatter_plan_apply_multi): exported, bound with the header's arity, and refusing bad call shapes before touching the device."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pn2_sa_hoist_rows_multi_bn", "pn2_scatter_plan_apply_multi")


def _header_arity(name):
    from pn2_amd import _abi
    return len(_abi.load(os.path.join(ROOT, "include", "pn2_abi.h")).functions[name].argnames)


def test_library_exports_and_binds_the_multi_scale_entry_points(pn2):
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pn2._lib.SIGNATURES, name
        assert len(pn2._lib.SIGNATURES[name]) == _header_arity(name), name
    assert _header_arity("pn2_sa_hoist_rows_multi_bn") == 30 and _header_arity("pn2_scatter_plan_apply_multi") == 14
    # the statistics epilogue updates moving averages: never launched twice by the duplicate-launch hook
    assert "pn2_sa_hoist_rows_multi_bn" in pn2._lib._STATEFUL


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _ptrs(*v):
    return (ctypes.c_void_p * len(v))(*v)


def _sizes(*v):
    return (ctypes.c_size_t * len(v))(*v)


def test_hoist_multi_argument_validation_needs_no_gpu(pn2):
    L = pn2._lib.lib
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    nul = None

    def call(nscales, couts, zcols=None, z_stride=128, z=fake, finish=None, ws=None):
        n = max(len(couts), 1)
        couts = list(couts) or [4]
        zcols = zcols if zcols is not None else [sum(couts[:i]) for i in range(n)]
        tab = _ptrs(*([4096] * n))
        return L.pn2_sa_hoist_rows_multi_bn(nscales, 2, 64, 8, z_stride, fake, fake, z, _ints(*([4] * n)), _ints(*couts), _ints(*zcols),
                                            tab, tab, tab, nul, ws if ws is not None else tab, _sizes(*([1 << 30] * n)),
                                            finish if finish is not None else _ints(*([0] * n)), nul, nul, nul, 1e-3, 0.9, nul, nul,
                                            nul, nul, nul, nul, nul)

    assert call(0, [4]) == -1                       # PN2_EINVAL: nscales in 1..4
    assert call(5, [4, 4, 4, 4, 4]) == -1
    assert call(-1, [4]) == -1
    assert call(1, [6]) == -4                       # PN2_EUNSUP: cout % 4
    assert call(3, [4, 32, 70]) == -4
    assert call(1, [1028], z_stride=2048) == -4     # cout <= 1024
    assert call(2, [4, 8], zcols=[0, 2]) == -1      # a column block that does not start on 16 bytes
    assert call(2, [64, 128], z_stride=128) == -1   # ... or leaves z
    assert call(1, [4], z_stride=126) == -1
    assert call(1, [4], z=nul) == -2                # PN2_ENULL
    assert call(1, [4], z=ctypes.c_void_p(4100)) == -1   # 16-byte aligned operands
    assert call(1, [4], finish=_ints(3)) == -1      # finish in 0..2
    assert call(1, [4], finish=_ints(2)) == -2      # finish 2 needs gamma / beta / save_mean / save_invstd
    assert call(1, [4], ws=_ptrs(None)) == -2       # every scale has a workspace
    assert L.pn2_sa_hoist_rows_multi_bn(1, 2, 64, 8, 4, fake, fake, fake, nul, nul, nul, nul, nul, nul, nul, nul, nul, nul, nul, nul,
                                        nul, 1e-3, 0.9, nul, nul, nul, nul, nul, nul, nul) == -2


def test_scatter_apply_multi_argument_validation_needs_no_gpu(pn2):
    L = pn2._lib.lib
    fake = ctypes.c_void_p(4096)
    nul = None

    def call(nplans, cs, ocols=None, out_stride=128, out=fake, in_stride=None, nent=64, rows=4096):
        n = max(len(cs), 1)
        cs = list(cs) or [4]
        ocols = ocols if ocols is not None else [sum(cs[:i]) for i in range(n)]
        tab = _ptrs(*([rows] * n))
        return L.pn2_scatter_plan_apply_multi(nplans, 2, 16, out_stride, _ints(*([nent] * n)), _ints(*([1] * n)), _ints(*cs),
                                              _ints(*ocols), tab, _ints(*(in_stride or cs)), _ptrs(*([4096] * n)),
                                              _sizes(*([1 << 30] * n)), out, nul)

    assert call(0, [4]) == -1                       # PN2_EINVAL: nplans in 1..4
    assert call(5, [4, 4, 4, 4, 4]) == -1
    assert call(1, [6]) == -4                       # PN2_EUNSUP: c % 4
    assert call(2, [32, 70]) == -4
    assert call(1, [1028], out_stride=2048) == -4
    assert call(2, [8, 8], ocols=[0, 4]) == -1      # overlapping column blocks
    assert call(2, [8, 8], ocols=[0, 10]) == -1     # a block that does not start on 16 bytes
    assert call(2, [64, 128], out_stride=128) == -1  # a block that leaves out
    assert call(1, [8], in_stride=[4]) == -1        # in_stride >= c
    assert call(1, [4], out=nul) == -2              # PN2_ENULL
    assert call(1, [4], out=ctypes.c_void_p(4100)) == -4   # as pn2_scatter_plan_apply: out 16-byte aligned
    assert call(1, [4], rows=4098) == -4            # rows_in 4-byte aligned
    assert L.pn2_scatter_plan_apply_multi(1, 2, 16, 4, nul, nul, nul, nul, nul, nul, nul, nul, fake, nul) == -2
    # a plan shorter than pn2_scatter_plan_bytes
    assert L.pn2_scatter_plan_apply_multi(1, 2, 16, 4, _ints(64), _ints(1), _ints(4), _ints(0), _ptrs(4096), _ints(4), _ptrs(4096),
                                          _sizes(8), fake, nul) == -1
