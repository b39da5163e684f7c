"""The int8 entry points' public surface, checked without a GPU:
the functions are declared in include/tcsc_gpu.h, exported and bound; each
answers a NULL plan or NULL pointers with TCSC_E_ARG and a message before any
HIP call (so on a host with no device at all); and the int8 MFMA workspace
never exceeds the fp32 call's for the same shape, which is why
tcsc_gpu_plan_reserve covers int8 launches as it is."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tcsc_amd
from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("tcsc_gpu_plan_enable_i8", "tcsc_gpu_plan_has_i8", "tcsc_gpu_sgemm_i8", "tcsc_gpu_launch_info_i8",
               "tcsc_gpu_quantize_rows_i8")

# a non-NULL "device pointer" that is never dereferenced
FAKE = 0x1000
E_ARG = 1


@pytest.fixture(scope="module")
def built_lib():
    tcsc_amd.build()
    return tcsc_amd.lib()


def last_error():
    return tcsc_amd.last_error()


def test_symbols_are_declared_listed_and_bind(built_lib):
    header = open(os.path.join(ROOT, "include", "tcsc_gpu.h")).read()
    for name in NEW_SYMBOLS + ("tcsc_gpu_workspace_bound_i8",):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in tcsc_gpu.h"
        assert name in tcsc_amd.EXPORTED_SYMBOLS, name
        assert getattr(built_lib, name).argtypes is not None, name
    # the sgemm takes the fp32 call's arguments plus the scale pointer
    assert len(built_lib.tcsc_gpu_sgemm_i8.argtypes) == len(built_lib.tcsc_gpu_sgemm.argtypes) + 1
    assert len(built_lib.tcsc_gpu_launch_info_i8.argtypes) == len(built_lib.tcsc_gpu_launch_info.argtypes)


def test_python_surface():
    for name in ("enable_i8", "sgemm_i8", "launch_info_i8"):
        assert callable(getattr(tcsc_amd.Plan, name))
    assert isinstance(tcsc_amd.Plan.has_i8, property)
    assert callable(tcsc_amd.quantize_rows_i8)


def null_plan():
    plan = tcsc_amd.Plan.__new__(tcsc_amd.Plan)
    plan.handle = None
    return plan


def test_enable_and_has_i8_reject_a_null_plan(built_lib):
    assert built_lib.tcsc_gpu_plan_enable_i8(None, None) == E_ARG
    assert "tcsc_gpu_plan_enable_i8" in last_error()
    assert built_lib.tcsc_gpu_plan_has_i8(None) == 0
    assert "tcsc_gpu_plan_has_i8" in last_error()
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_plan_enable_i8"):
        null_plan().enable_i8()


@pytest.mark.parametrize("M,ldy,variant", [(4, 8, 2), (-1, 8, 2), (4, 8, 6), (4, 8, -1)])
def test_sgemm_i8_rejects_bad_arguments_without_a_gpu(built_lib, M, ldy, variant):
    p = C.c_void_p(FAKE)
    assert built_lib.tcsc_gpu_sgemm_i8(None, p, p, p, p, M, ldy, variant, 0.2, None) == E_ARG
    assert "tcsc_gpu_sgemm_i8" in last_error()
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_sgemm_i8"):
        null_plan().sgemm_i8(FAKE, None, FAKE, FAKE, 4, 8, "prelu_basic", 0.2)


def test_launch_info_i8_rejects_bad_arguments_without_a_gpu(built_lib):
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_launch_info_i8"):
        null_plan().launch_info_i8(4)
    path, slices = C.c_int(), C.c_int()
    assert built_lib.tcsc_gpu_launch_info_i8(None, -1, C.byref(path), C.byref(slices)) == E_ARG
    assert built_lib.tcsc_gpu_launch_info_i8(None, 4, None, None) == E_ARG


def test_quantize_rows_i8_rejects_bad_arguments_without_a_gpu(built_lib):
    p = C.c_void_p(FAKE)
    q = built_lib.tcsc_gpu_quantize_rows_i8
    assert q(None, 4, 8, p, p, None) == E_ARG and "tcsc_gpu_quantize_rows_i8" in last_error()   # NULL X
    assert q(p, 4, 8, None, p, None) == E_ARG                                                    # NULL Xq
    assert q(p, 4, 8, p, None, None) == E_ARG                                                    # NULL scale
    assert q(p, -1, 8, p, p, None) == E_ARG and q(p, 4, -1, p, p, None) == E_ARG                 # negative sizes
    assert q(None, 0, 8, None, None, None) == 0                                                  # M = 0: nothing to do
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_quantize_rows_i8"):
        tcsc_amd.quantize_rows_i8(None, FAKE, FAKE, 4, 8)


def bound(lib, M, K, N):
    i8, f32 = C.c_size_t(), C.c_size_t()
    assert lib.tcsc_gpu_workspace_bound_i8(M, K, N, C.byref(i8), C.byref(f32)) == 0
    return i8.value, f32.value


# the sweep: small and ragged M, every K residue class that changes a block count, N around the tile widths
Ms = [1, 4, 5, 17, 63, 64, 65, 96, 127, 128, 129, 200, 256, 257, 1000, 2048, 4097]
Ks = [1, 63, 64, 65, 127, 128, 129, 300, 511, 512, 513, 1023, 1100, 2047, 2048, 2049, 3000, 4095, 8192, 8193, 16384,
      20000, 100003]
Ns = [1, 64, 130, 255, 256, 257, 300, 512, 600, 1024, 4096, 8192, 16384]


@pytest.mark.parametrize("wgs", [None, "0", "64", "4096"])
def test_int8_workspace_never_exceeds_the_fp32_calls(built_lib, monkeypatch, wgs):
    """The int8 MFMA workspace <= the fp32 call's (mfma_ws, csrc/tcsc_api.cpp) over the sweep, whatever
    $TCSC_MFMA_WGS asks of the two K splits."""
    if wgs is None:
        monkeypatch.delenv("TCSC_MFMA_WGS", raising=False)
    else:
        monkeypatch.setenv("TCSC_MFMA_WGS", wgs)
    splits = 0
    for M in Ms:
        for K in Ks:
            for N in Ns:
                i8, f32 = bound(built_lib, M, K, N)
                assert 0 < i8 <= f32, (M, K, N, i8, f32)
                # X8 alone: M rows of K rounded up to 128 bytes, rounded up to 256
                x8 = (M * ((K + 127) // 128 * 128) + 255) // 256 * 256
                assert i8 >= x8 and (i8 - x8) % (4 * M * N) == 0, (M, K, N)
                splits += i8 > x8
    if wgs == "0":
        assert splits == 0
    else:
        assert splits > 0  # the sweep reaches shapes whose K is split


@pytest.mark.parametrize("wgs", [None, "0", "64", "4096"])
def test_workspace_bound_equals_the_recorded_sweep(built_lib, monkeypatch, wgs):
    """Both sizes over the same sweep are what the per-type workspace layouts gave before they became one function
    (tests/golden/routing/i8_workspace_bound.npz, written by tests/golden/gen_routing.py --bound)."""
    if wgs is None:
        monkeypatch.delenv("TCSC_MFMA_WGS", raising=False)
    else:
        monkeypatch.setenv("TCSC_MFMA_WGS", wgs)
    z = np.load(os.path.join(GOLDEN, "routing", "i8_workspace_bound.npz"))
    assert list(z["Ms"]) == Ms and list(z["Ks"]) == Ks and list(z["Ns"]) == Ns
    recorded = z["wgs_" + (wgs or "unset")]
    got = np.array([[[bound(built_lib, M, K, N) for N in Ns] for K in Ks] for M in Ms], np.int64)
    bad = np.argwhere((got != recorded).any(axis=-1))
    assert bad.size == 0, (f"{len(bad)} shapes differ, first M={Ms[bad[0][0]]} K={Ks[bad[0][1]]} N={Ns[bad[0][2]]}: "
                           f"{got[tuple(bad[0])]} (recorded {recorded[tuple(bad[0])]})")


def test_workspace_bound_rejects_bad_shapes(built_lib):
    assert built_lib.tcsc_gpu_workspace_bound_i8(-1, 8, 8, None, None) == E_ARG
    assert built_lib.tcsc_gpu_workspace_bound_i8(4, 0, 8, None, None) == E_ARG
    assert "tcsc_gpu_workspace_bound_i8" in last_error()
