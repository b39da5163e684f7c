"""The packed plan's public surface, checked without a GPU: the new functions are declared in
include/tcsc_gpu.h, listed, exported and bound; the entry points that take a plan answer a NULL one with TCSC_E_ARG
and a message before any HIP call, and so do the constructors for arguments they can refuse on the host; the Python
surface exists.  What a packed plan computes is tests/test_gpu_packed.py's."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import tcsc_amd
from conftest import ROOT

NEW_SYMBOLS = ("tcsc_gpu_plan_create_packed", "tcsc_gpu_plan_create_packed_device", "tcsc_gpu_plan_is_packed",
               "tcsc_gpu_plan_copy_w2")
E_ARG = 1


@pytest.fixture(scope="module")
def built_lib():
    tcsc_amd.build()
    return tcsc_amd.lib()


def test_symbols_are_declared_listed_exported_and_bind(built_lib):
    header = open(os.path.join(ROOT, "include", "tcsc_gpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", tcsc_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in tcsc_gpu.h"
        assert name in tcsc_amd.EXPORTED_SYMBOLS, name
        assert name in exported, name
        assert getattr(built_lib, name).argtypes is not None, name
    # the device constructor takes tcsc_gpu_plan_create_device's argument list
    assert built_lib.tcsc_gpu_plan_create_packed_device.argtypes == built_lib.tcsc_gpu_plan_create_device.argtypes
    assert built_lib.tcsc_gpu_plan_create_packed.argtypes == built_lib.tcsc_gpu_plan_create.argtypes


def test_null_plans_are_refused_before_any_hip_call(built_lib):
    assert built_lib.tcsc_gpu_plan_is_packed(None) == 0
    assert "tcsc_gpu_plan_is_packed" in tcsc_amd.last_error()
    assert built_lib.tcsc_gpu_plan_copy_w2(None, None, 0, None) == E_ARG
    assert "tcsc_gpu_plan_copy_w2" in tcsc_amd.last_error()
    plan = tcsc_amd.Plan.__new__(tcsc_amd.Plan)
    plan.handle = None
    assert plan.is_packed is False
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_plan_copy_w2"):
        plan.copy_w2(0)


def test_constructors_refuse_bad_arguments_on_the_host(built_lib):
    """NULL W or out, a column range outside W, K >= 2^22 and a reference-order request: TCSC_E_ARG and a message
    that names the call, with no device needed to say so."""
    h = C.c_void_p()
    assert built_lib.tcsc_gpu_plan_create_packed(None, 0, 0, 0, None, C.byref(h)) == E_ARG
    assert "tcsc_gpu_plan_create_packed" in tcsc_amd.last_error()
    assert built_lib.tcsc_gpu_plan_create_packed_device(4, 4, None, None, None, None, 0, 4, 0, None, C.byref(h)) == E_ARG
    assert "tcsc_gpu_plan_create_packed_device" in tcsc_amd.last_error()
    W = tcsc_amd.TcscMatrix.from_dense(np.eye(4, dtype=np.float32))
    assert built_lib.tcsc_gpu_plan_create_packed(W.ptr, 0, 4, 0, None, None) == E_ARG
    assert built_lib.tcsc_gpu_plan_create_packed(W.ptr, 2, 5, 0, None, C.byref(h)) == E_ARG
    assert built_lib.tcsc_gpu_plan_create_packed(W.ptr, 3, 2, 0, None, C.byref(h)) == E_ARG
    # K >= 2^22: the i32 sums of the int8 kernels could pass 2^31 (pointers that are never read: refused first)
    one = C.c_void_p(16)
    rc = built_lib.tcsc_gpu_plan_create_packed_device(1 << 22, 4, one, one, one, one, 0, 4, 0, None, C.byref(h))
    assert rc == E_ARG and "K" in tcsc_amd.last_error() and not h.value
    # the reference order has no packed form
    tcsc_amd.set_order("reference")
    try:
        assert built_lib.tcsc_gpu_plan_create_packed(W.ptr, 0, 4, 0, None, C.byref(h)) == E_ARG
        assert "reference" in tcsc_amd.last_error() and not h.value
        with pytest.raises(tcsc_amd.TcscError, match="reference"):
            tcsc_amd.Plan.packed(W)
    finally:
        tcsc_amd.set_order("fast")
    # a row index outside [0, K) is found by the host check, as tcsc_gpu_plan_create finds it
    bad = tcsc_amd.TcscMatrix.from_arrays(4, 2, [0, 1, 2], [0, 0, 0], [1, 4], [])
    assert built_lib.tcsc_gpu_plan_create_packed(bad.ptr, 0, 2, 0, None, C.byref(h)) == E_ARG
    assert "row_index_pos" in tcsc_amd.last_error()
    bad.free()
    W.free()


def test_python_surface():
    assert callable(tcsc_amd.Plan.packed) and callable(tcsc_amd.Plan.packed_from_device)
    assert isinstance(tcsc_amd.Plan.is_packed, property)
    assert callable(tcsc_amd.Plan.copy_w2)
    sig = inspect.signature(tcsc_amd.Plan.packed)
    assert list(sig.parameters) == ["W", "col_begin", "col_end", "device", "stream"]
    import tcsc_amd.nn as nn

    assert "PackedTernaryLinear" in nn.__all__
    src = inspect.getsource(nn)
    assert "class PackedTernaryLinear" in src and "Plan.packed" in src and "def reserve(self, max_rows" in src
    with pytest.raises(tcsc_amd.TcscError, match="freed"):
        freed = tcsc_amd.TcscMatrix.from_dense(np.eye(2, dtype=np.float32))
        freed.free()
        tcsc_amd.Plan.packed(freed)


def test_a_packed_plan_cannot_be_made_without_a_device(built_lib):
    if tcsc_amd.device_count() > 0:
        pytest.skip("GPU present")
    W = tcsc_amd.TcscMatrix.from_dense(np.eye(4, dtype=np.float32))
    with pytest.raises(tcsc_amd.TcscError):
        tcsc_amd.Plan.packed(W)
    W.free()
