"""CPU tests of pn2_label_confusion (csrc/pn2_metric.hip): the entry point is bound from the header and refuses bad arguments
before any HIP call (no GPU needed)."""
import ctypes


def test_label_confusion_is_bound_from_the_header(pn2):
    i, p, ll = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    assert pn2._lib.SIGNATURES["pn2_label_confusion"] == [ll, i, p, p, i, p, p, p]
    f = pn2._lib.ABI.functions["pn2_label_confusion"]
    assert f.restype is i
    assert f.argnames == ("n", "num_class", "gt", "pd", "label64", "confusion", "dropped", "stream")
    assert "pn2_label_confusion" not in pn2._lib._TRACE_ARGS
    assert pn2._lib.ABI.constants["PN2_ABI_VERSION"] == 2


def test_label_confusion_argument_checks_need_no_gpu(pn2):
    L = pn2._lib.lib
    nul = None
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    EINVAL, ENULL, EUNSUP = -1, -2, -4
    for l64 in (0, 1):
        assert L.pn2_label_confusion(0, 9, fake, fake, l64, fake, fake, nul) == EINVAL      # n > 0
        assert L.pn2_label_confusion(-7, 9, fake, fake, l64, fake, nul, nul) == EINVAL
        assert L.pn2_label_confusion(10, 0, fake, fake, l64, fake, fake, nul) == EINVAL     # num_class > 0
        assert L.pn2_label_confusion(10, -1, fake, fake, l64, fake, fake, nul) == EINVAL
        assert L.pn2_label_confusion(10, 65, fake, fake, l64, fake, fake, nul) == EUNSUP    # above 64 classes
        assert L.pn2_label_confusion(10, 9, nul, fake, l64, fake, fake, nul) == ENULL       # gt
        assert L.pn2_label_confusion(10, 9, fake, nul, l64, fake, fake, nul) == ENULL       # pd
        assert L.pn2_label_confusion(10, 9, fake, fake, l64, nul, fake, nul) == ENULL       # confusion
        # beyond 2^39 pairs a workgroup's uint32 bin could overflow: refused (the bound itself is accepted, see the GPU tests
        # for sizes that run)
        assert L.pn2_label_confusion((1 << 39) + 1, 9, fake, fake, l64, fake, fake, nul) == EINVAL
    # the checks come in the documented order: a bad count wins over the class limit, the class limit over a NULL pointer
    assert L.pn2_label_confusion(0, 65, nul, nul, 0, nul, nul, nul) == EINVAL
    assert L.pn2_label_confusion(10, 65, nul, nul, 0, nul, nul, nul) == EUNSUP


def test_label_confusion_helper_refuses_cpu_tensors(pn2):
    import pytest
    import torch
    with pytest.raises(ValueError, match="MI355X only"):
        pn2.util.metric.label_confusion(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32),
                                        torch.zeros(9, dtype=torch.int64))
