"""The decode path's public surface, checked without a GPU: the
new functions are declared in include/tcsc_gpu.h, exported and bound; the image
size and the default routing rule are host arithmetic and follow their formulas;
the entry points that need a plan answer a NULL one with TCSC_E_ARG and a
message before any HIP call.

k_decode8 reads X in place (guarded byte loads where X is not 16-B aligned or
K % 16 != 0), so the path needs no workspace: nothing here bounds one against the
gather's, and tests/test_gpu_decode.py checks on a live plan that
tcsc_gpu_plan_workspace reports 0 for it."""
import ctypes as C
import os
import re

import pytest

import tcsc_amd
from conftest import ROOT

NEW_SYMBOLS = ("tcsc_gpu_plan_enable_w2", "tcsc_gpu_plan_has_w2", "tcsc_gpu_w2_image_bytes", "tcsc_gpu_decode_pays")
E_ARG = 1


@pytest.fixture(scope="module")
def built_lib():
    tcsc_amd.build()
    return tcsc_amd.lib()


def test_symbols_are_declared_listed_exported_and_bind(built_lib):
    import subprocess

    header = open(os.path.join(ROOT, "include", "tcsc_gpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", tcsc_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in tcsc_gpu.h"
        assert name in tcsc_amd.EXPORTED_SYMBOLS, name
        assert name in exported, name
        assert getattr(built_lib, name).argtypes is not None, name
    assert re.search(r"\bTCSC_PATH_DECODE\s*=\s*4\b", header)


def test_python_surface():
    assert callable(tcsc_amd.Plan.enable_w2)
    assert isinstance(tcsc_amd.Plan.has_w2, property)
    assert tcsc_amd.Plan.PATH_ID["decode"] == 4
    assert callable(tcsc_amd.w2_image_bytes) and callable(tcsc_amd.decode_pays)
    import inspect

    import tcsc_amd.nn as nn

    src = inspect.getsource(nn)
    assert "decode: bool = False" in src and "enable_w2" in src


def null_plan():
    plan = tcsc_amd.Plan.__new__(tcsc_amd.Plan)
    plan.handle = None
    return plan


def test_enable_and_has_w2_reject_a_null_plan(built_lib):
    """The GPU entry points fail loudly, before any HIP call (so on a host with no device at all)."""
    assert built_lib.tcsc_gpu_plan_enable_w2(None, None) == E_ARG
    assert "tcsc_gpu_plan_enable_w2" in tcsc_amd.last_error()
    assert built_lib.tcsc_gpu_plan_has_w2(None) == 0
    assert "tcsc_gpu_plan_has_w2" in tcsc_amd.last_error()
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_plan_enable_w2"):
        null_plan().enable_w2()
    need = C.c_size_t()
    assert built_lib.tcsc_gpu_plan_workspace(None, 4, 4, C.byref(need), None) == E_ARG


def test_a_plan_cannot_be_made_without_a_device(built_lib):
    import numpy as np

    if tcsc_amd.device_count() > 0:
        pytest.skip("GPU present")
    W = tcsc_amd.TcscMatrix.from_dense(np.eye(4, dtype=np.float32))
    with pytest.raises(tcsc_amd.TcscError):
        tcsc_amd.Plan(W).enable_w2()
    W.free()


Ks = [1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 4096, 4112, 6912, 8192, 100003, (1 << 22) - 1]
Ns = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 2560, 6912, 8192, 100003]


def test_image_bytes_follow_the_formula(built_lib):
    for K in Ks:
        for N in Ns:
            want = ((N + 15) // 16) * ((K + 255) // 256) * 1024
            assert tcsc_amd.w2_image_bytes(K, N) == want, (K, N)
    assert tcsc_amd.w2_image_bytes(8192, 8192) == 8192 * 8192 // 4  # a quarter byte per weight, no padding
    assert tcsc_amd.w2_image_bytes(0, 8) == 0 and tcsc_amd.w2_image_bytes(8, 0) == 0
    b = C.c_size_t()
    assert built_lib.tcsc_gpu_w2_image_bytes(-1, 8, C.byref(b)) == E_ARG
    assert built_lib.tcsc_gpu_w2_image_bytes(8, -1, C.byref(b)) == E_ARG
    assert built_lib.tcsc_gpu_w2_image_bytes(8, 8, None) == E_ARG
    assert "tcsc_gpu_w2_image_bytes" in tcsc_amd.last_error()


def small_m_fits(M, K):
    """The small-M path's LDS rule (csrc/tcsc_internal.h): M row pairs of 2 Kp floats, Kp = K + 1 rounded up to 4,
    in 160 KiB; M <= 4."""
    return 1 <= M <= 4 and M * 2 * ((K + 4) & ~3) * 4 <= 160 * 1024


def rule(M, K, N, nnz):
    return 1 <= M <= 16 and (M > 4 or not small_m_fits(M, K) or 16 * nnz > K * N)


def test_decode_pays_follows_its_rule():
    K = N = 4096
    edge = K * N // 16
    for M in (0, 1, 4, 5, 16, 17):
        for nnz in (0, edge - 1, edge, edge + 1, K * N):
            assert tcsc_amd.decode_pays(M, K, N, nnz) == rule(M, K, N, nnz), (M, nnz)
    # the clauses one by one
    assert not tcsc_amd.decode_pays(0, K, N, K * N) and not tcsc_amd.decode_pays(17, K, N, K * N)
    assert not tcsc_amd.decode_pays(1, K, N, edge) and tcsc_amd.decode_pays(1, K, N, edge + 1)
    assert not tcsc_amd.decode_pays(4, K, N, edge) and tcsc_amd.decode_pays(4, K, N, edge + 1)
    assert tcsc_amd.decode_pays(5, K, N, 0) and tcsc_amd.decode_pays(16, K, N, 0)
    # K = 16384: M = 4 does not fit the small-M path's LDS (M = 1 does), so a sparse W decodes at 4 and not at 1
    assert small_m_fits(1, 16384) and not small_m_fits(4, 16384)
    assert tcsc_amd.decode_pays(4, 16384, N, 0) and not tcsc_amd.decode_pays(1, 16384, N, 0)
    # a sweep against the restated rule, with K N beyond 2^31
    for M in (1, 2, 3, 4, 5, 16):
        for K_ in (1, 256, 4112, 10000, 16384, 20476, 20480, 65536):
            for N_ in (1, 16, 8192, 65536):
                for nnz in (0, K_ * N_ // 16, K_ * N_ // 16 + 1, K_ * N_):
                    assert tcsc_amd.decode_pays(M, K_, N_, nnz) == rule(M, K_, N_, nnz), (M, K_, N_, nnz)
