"""The public surface of the int8 calls with column scales and a typed Y, checked without a GPU:
tcsc_gpu_sgemm_i8_out and tcsc_gpu_sgemm_q8_out are declared in include/tcsc_gpu.h with the documented signatures,
exported and bound, beside enum tcsc_ytype; Plan.sgemm_i8 / sgemm_q8 take col_scale and ytype; the new argument
checks answer TCSC_E_ARG with a message naming the call before any HIP call (so on a host with no device); and
ternarize_absmean, which is host arithmetic, gives the bits of a literal numpy restatement of its rule.

A plan cannot exist without a device: the refusals that need a live plan (a bf16 Y or a column scale on the
gather route, ytype 2 and a NULL Y on a live plan) are in tests/test_gpu_out.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import tcsc_amd
from conftest import ROOT

FAKE = 0x1000  # a non-NULL "device pointer" that is never dereferenced
E_ARG = 1

SIGNATURES = {
    "tcsc_gpu_sgemm_i8_out": "const tcsc_gpu_plan *plan, const void *dXq, const float *dScale, "
                             "const float *dColScale, const float *dB, void *dY, int ytype, "
                             "int M, int ldy, int variant, float a, void *stream",
    "tcsc_gpu_sgemm_q8_out": "const tcsc_gpu_plan *plan, const void *dX, int xtype, void *dXq, "
                             "float *dScale, const float *dColScale, const float *dB, void *dY, "
                             "int ytype, int M, int ldy, int variant, float a, void *stream",
}


@pytest.fixture(scope="module")
def built_lib():
    tcsc_amd.build()
    return tcsc_amd.lib()


def null_plan():
    plan = tcsc_amd.Plan.__new__(tcsc_amd.Plan)
    plan.handle = None
    return plan


def test_symbols_are_declared_with_their_signatures_exported_and_bind(built_lib):
    header = open(os.path.join(ROOT, "include", "tcsc_gpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", tcsc_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, sig in SIGNATURES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} not declared in tcsc_gpu.h"
        assert " ".join(m.group(1).split()) == sig, name
        assert name in tcsc_amd.EXPORTED_SYMBOLS, name
        assert name in exported, name
        assert len(getattr(built_lib, name).argtypes) == sig.count(",") + 1, name
    assert re.search(r"enum\s+tcsc_ytype\s*\{\s*TCSC_Y_F32\s*=\s*0\s*,\s*TCSC_Y_BF16\s*=\s*1\s*\}", header)


def test_python_surface():
    assert tcsc_amd.YTYPE_ID == {"f32": 0, "bf16": 1}
    for method in (tcsc_amd.Plan.sgemm_i8, tcsc_amd.Plan.sgemm_q8):
        params = inspect.signature(method).parameters
        assert params["col_scale"].default is None and params["ytype"].default is None, method
    assert callable(tcsc_amd.ternarize_absmean)


@pytest.mark.parametrize("ytype,Y,B", [(2, FAKE, FAKE), (-1, FAKE, FAKE), (0, None, FAKE), (1, None, FAKE),
                                       (0, FAKE, None), (1, FAKE, None), (0, FAKE, FAKE), (1, FAKE, FAKE)])
@pytest.mark.parametrize("M", [4, 0])
def test_out_calls_reject_bad_arguments_without_a_gpu(built_lib, ytype, Y, B, M):
    """ytype 2 and -1, a NULL Y and a NULL B, each on a NULL plan (and the NULL plan alone): TCSC_E_ARG naming the call."""
    p = C.c_void_p(FAKE)
    for cs in (None, p):
        assert built_lib.tcsc_gpu_sgemm_i8_out(None, p, p, cs, B, Y, ytype, M, 8, 2, 0.2, None) == E_ARG
        assert "tcsc_gpu_sgemm_i8_out" in tcsc_amd.last_error()
        for xtype in (0, 1):
            assert built_lib.tcsc_gpu_sgemm_q8_out(None, p, xtype, p, p, cs, B, Y, ytype, M, 8, 2, 0.2, None) == E_ARG
            assert "tcsc_gpu_sgemm_q8_out" in tcsc_amd.last_error()


def test_out_messages_say_what_is_wrong(built_lib):
    p = C.c_void_p(FAKE)
    for call, args in ((built_lib.tcsc_gpu_sgemm_i8_out, (p, p)), (built_lib.tcsc_gpu_sgemm_q8_out, (p, 1, p, p))):
        assert call(None, *args, None, p, p, 2, 4, 8, 2, 0.2, None) == E_ARG and "ytype=2" in tcsc_amd.last_error()
        assert call(None, *args, None, p, p, -1, 4, 8, 2, 0.2, None) == E_ARG and "ytype=-1" in tcsc_amd.last_error()
        assert call(None, *args, None, p, p, 1, 4, 8, 2, 0.2, None) == E_ARG and "NULL plan" in tcsc_amd.last_error()


def test_plan_methods_go_through_the_out_calls():
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_sgemm_i8_out"):
        null_plan().sgemm_i8(FAKE, FAKE, FAKE, FAKE, 4, 8, "prelu_basic", 0.2, col_scale=FAKE, ytype="bf16")
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_sgemm_q8_out"):
        null_plan().sgemm_q8(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, "prelu_basic", 0.2, xtype="bf16", col_scale=FAKE,
                             ytype="bf16")
    with pytest.raises(tcsc_amd.TcscError, match=r"ytype=2"):
        null_plan().sgemm_i8(FAKE, FAKE, FAKE, FAKE, 4, 8, ytype=2)
    with pytest.raises(tcsc_amd.TcscError, match="fp32 or bf16"):
        null_plan().sgemm_q8(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, ytype="int8")


def absmean_restated(W):
    """The rule of the issue, literally: beta = mean |W| in fp32, T = clip(rint(W / beta), -1, 1)."""
    W = np.asarray(W, dtype=np.float32)
    beta = np.abs(W).mean(dtype=np.float32)
    if beta == 0:
        return np.zeros(W.shape, np.int8), np.float32(0)
    return np.clip(np.rint(W / beta), -1, 1).astype(np.int8), np.float32(beta)


def check_absmean(W):
    T, beta = tcsc_amd.ternarize_absmean(W)
    Tr, br = absmean_restated(W)
    assert isinstance(T, np.ndarray) and T.dtype == np.int8 and T.shape == np.shape(W)
    assert np.asarray(beta).dtype == np.float32
    assert np.float32(beta).tobytes() == br.tobytes()
    assert np.array_equal(T, Tr)
    return T, float(beta)


def test_ternarize_absmean_on_a_normal_matrix():
    W = np.random.default_rng(2101).standard_normal((37, 19)).astype(np.float32)
    T, beta = check_absmean(W)
    assert set(np.unique(T)) == {-1, 0, 1} and 0.7 < beta < 0.9  # E|N(0,1)| = 0.798
    check_absmean(W.astype(np.float64))  # other float types are taken as fp32


def test_ternarize_absmean_on_zeros():
    T, beta = check_absmean(np.zeros((5, 7), np.float32))
    assert beta == 0.0 and not T.any()


def test_ternarize_absmean_ties():
    """Entries at exactly +-0.5 beta and +-1.5 beta: rint rounds halves to even, so 0 and +-2 -> clip +-1.  Two
    entries each of +-0.5 and +-1.5 have mean |w| = 1 exactly, and every quotient is exact."""
    W = np.array([[0.5, -0.5, 1.5, -1.5], [-1.5, 1.5, -0.5, 0.5]], np.float32)
    T, beta = check_absmean(W)
    assert beta == 1.0
    assert np.array_equal(T, np.array([[0, 0, 1, -1], [-1, 1, 0, 0]], np.int8))
    T, beta = check_absmean(W * np.float32(0.25))  # a power of two keeps everything exact
    assert beta == 0.25 and np.array_equal(T, np.array([[0, 0, 1, -1], [-1, 1, 0, 0]], np.int8))
