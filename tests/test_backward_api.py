"""The backward pass's public surface, checked without a GPU: the new symbols
are declared, exported and bound, and the argument checks of
tcsc_gpu_prelu_backward / tcsc_gpu_sgemm_t answer TCSC_E_ARG before any HIP
call (so they answer on a host with no device at all)."""
import importlib

import pytest

import tcsc_amd

NEW_SYMBOLS = ("tcsc_gpu_transpose_index", "tcsc_gpu_plan_create_transposed",
               "tcsc_gpu_plan_create_transposed_device", "tcsc_gpu_sgemm_t", "tcsc_gpu_prelu_backward")


@pytest.fixture(scope="module")
def built_lib():
    tcsc_amd.build()
    return tcsc_amd.lib()


def test_new_symbols_are_listed_and_bind(built_lib):
    for name in NEW_SYMBOLS:
        assert name in tcsc_amd.EXPORTED_SYMBOLS, name
        fn = getattr(built_lib, name)
        assert fn.argtypes is not None, name
    for name in ("gpu_transpose_index", "prelu_backward"):
        assert callable(getattr(tcsc_amd, name))
    for name in ("transposed", "transposed_from_device", "sgemm_t"):
        assert callable(getattr(tcsc_amd.Plan, name))


# a non-NULL "device pointer" that is never dereferenced: every call below must be
# refused by the argument check, before any HIP call
FAKE = 0x1000


@pytest.mark.parametrize("kwargs,what", [
    (dict(G=FAKE, Y=FAKE, DZ=FAKE, DB=FAKE, M=4, N=8, ldg=7), "ldg < N"),
    (dict(G=FAKE, Y=FAKE, DZ=FAKE, DB=FAKE, M=4, N=8, ldy=7), "ldy < N"),
    (dict(G=FAKE, Y=FAKE, DZ=FAKE, DB=FAKE, M=4, N=8, lddz=5), "lddz < N"),
    (dict(G=FAKE, Y=FAKE, DZ=FAKE, DB=FAKE, M=-1, N=8), "negative M"),
    (dict(G=FAKE, Y=FAKE, DZ=FAKE, DB=FAKE, M=4, N=-8), "negative N"),
    (dict(G=None, Y=FAKE, DZ=FAKE, DB=FAKE, M=4, N=8), "NULL G"),
])
def test_prelu_backward_rejects_bad_arguments_without_a_gpu(built_lib, kwargs, what):
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)") as ei:
        tcsc_amd.prelu_backward(a=0.2, **kwargs)
    assert "tcsc_gpu_prelu_backward" in str(ei.value), what


def test_sgemm_t_rejects_a_null_plan_without_a_gpu(built_lib):
    plan = tcsc_amd.Plan.__new__(tcsc_amd.Plan)
    plan.handle = None
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*NULL plan"):
        plan.sgemm_t(FAKE, FAKE, 4, 8)


def test_transpose_entry_points_reject_bad_ranges_without_a_gpu(built_lib):
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)"):
        tcsc_amd.gpu_transpose_index(4, 8, FAKE, FAKE, FAKE, FAKE, 5, 3, FAKE, FAKE, FAKE, FAKE)
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)"):
        tcsc_amd.gpu_transpose_index(-1, 8, FAKE, FAKE, FAKE, FAKE, 0, 8, FAKE, FAKE, FAKE, FAKE)
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)"):
        tcsc_amd.gpu_transpose_index(4, 8, None, FAKE, FAKE, FAKE, 0, 8, FAKE, FAKE, FAKE, FAKE)
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)"):
        tcsc_amd.Plan.transposed_from_device(4, 8, FAKE, FAKE, FAKE, FAKE, 0, 9)


def test_nn_module_imports_without_a_gpu():
    nn = importlib.import_module("tcsc_amd.nn")
    assert "TernaryLinear" in nn.__all__
    with pytest.raises(AttributeError):
        nn.no_such_name
