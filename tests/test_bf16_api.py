"""The bf16 entry points' public surface, checked without a GPU:
tcsc_gpu_sgemm_bf16 and tcsc_gpu_launch_info_bf16 are declared in
include/tcsc_gpu.h, exported and bound, Plan has the two methods, and the
argument checks answer TCSC_E_ARG before any HIP call (so they answer on a
host with no device at all)."""
import ctypes as C
import os
import re

import pytest

import tcsc_amd
from conftest import ROOT

NEW_SYMBOLS = ("tcsc_gpu_sgemm_bf16", "tcsc_gpu_launch_info_bf16")

# a non-NULL "device pointer" that is never dereferenced
FAKE = 0x1000


@pytest.fixture(scope="module")
def built_lib():
    tcsc_amd.build()
    return tcsc_amd.lib()


def test_symbols_are_declared_listed_and_bind(built_lib):
    header = open(os.path.join(ROOT, "include", "tcsc_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in tcsc_gpu.h"
        assert name in tcsc_amd.EXPORTED_SYMBOLS, name
        fn = getattr(built_lib, name)
        assert fn.argtypes is not None, name
    assert len(built_lib.tcsc_gpu_sgemm_bf16.argtypes) == len(built_lib.tcsc_gpu_sgemm.argtypes)
    assert len(built_lib.tcsc_gpu_launch_info_bf16.argtypes) == len(built_lib.tcsc_gpu_launch_info.argtypes)


def test_plan_has_the_two_methods():
    for name in ("sgemm_bf16", "launch_info_bf16"):
        assert callable(getattr(tcsc_amd.Plan, name))


def null_plan():
    plan = tcsc_amd.Plan.__new__(tcsc_amd.Plan)
    plan.handle = None
    return plan


@pytest.mark.parametrize("M,variant,what", [
    (4, "prelu_basic", "NULL plan"),
    (-1, "prelu_basic", "negative M"),
])
def test_sgemm_bf16_rejects_bad_arguments_without_a_gpu(built_lib, M, variant, what):
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)") as ei:
        null_plan().sgemm_bf16(FAKE, FAKE, FAKE, M, 8, variant, 0.2)
    assert "tcsc_gpu_sgemm_bf16" in str(ei.value), what


def test_sgemm_bf16_rejects_a_bad_variant_without_a_gpu(built_lib):
    # straight through the C ABI: Plan.sgemm_bf16 names variants, the ABI numbers them
    for variant in (-1, 6, 99):
        rc = built_lib.tcsc_gpu_sgemm_bf16(None, C.c_void_p(FAKE), C.c_void_p(FAKE), C.c_void_p(FAKE), 4, 8, variant,
                                           0.2, None)
        assert rc == 1, variant  # TCSC_E_ARG


def test_launch_info_bf16_rejects_bad_arguments_without_a_gpu(built_lib):
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_launch_info_bf16"):
        null_plan().launch_info_bf16(4)
    path, slices = C.c_int(), C.c_int()
    assert built_lib.tcsc_gpu_launch_info_bf16(None, -1, C.byref(path), C.byref(slices)) == 1
    assert built_lib.tcsc_gpu_launch_info_bf16(None, 4, None, None) == 1
