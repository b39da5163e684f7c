"""The fused quantize-and-decode call's public surface, checked without a GPU: the four new
functions are declared in include/tcsc_gpu.h with the documented signatures, exported and bound; the fusing rule is
host arithmetic and follows its formula; the entry points answer bad arguments with TCSC_E_ARG and a message naming
the call before any HIP call (so on a host with no device at all).

A plan cannot exist without a device, so the checks that need a live plan behind them (a NULL X, scale, B or Y,
ldy < cols, a NULL dXq off the fused route) are in tests/test_gpu_q8.py; here every call is made on a NULL plan,
with each of the other faults beside it, and the bf16 quantizer, which takes no plan, gets each of its own."""
import ctypes as C
import os
import re
import subprocess

import pytest

import tcsc_amd
from conftest import ROOT

NEW_SYMBOLS = ("tcsc_gpu_quantize_rows_i8_bf16", "tcsc_gpu_sgemm_q8", "tcsc_gpu_launch_info_q8",
               "tcsc_gpu_quant_fuse_pays")
FAKE = 0x1000  # a non-NULL "device pointer" that is never dereferenced
E_ARG = 1

SIGNATURES = {
    "tcsc_gpu_quantize_rows_i8_bf16": "const void *dX_bf16, int M, int K, void *dXq, float *dScale, void *stream",
    "tcsc_gpu_sgemm_q8": "const tcsc_gpu_plan *plan, const void *dX, int xtype, void *dXq, float *dScale, "
                         "const float *dB, float *dY, int M, int ldy, int variant, float a, void *stream",
    "tcsc_gpu_launch_info_q8": "const tcsc_gpu_plan *plan, int M, int xtype, int *path, int *slices, int *fused",
    "tcsc_gpu_quant_fuse_pays": "int M, int K, int N, int xtype",
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
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} not declared in tcsc_gpu.h"
        assert " ".join(m.group(1).split()) == SIGNATURES[name], name
        assert name in tcsc_amd.EXPORTED_SYMBOLS, name
        assert name in exported, name
        assert len(getattr(built_lib, name).argtypes) == SIGNATURES[name].count(",") + 1, name
    assert re.search(r"enum\s+tcsc_xtype\s*\{\s*TCSC_X_F32\s*=\s*0\s*,\s*TCSC_X_BF16\s*=\s*1\s*\}", header)


def test_python_surface():
    assert callable(tcsc_amd.Plan.sgemm_q8) and callable(tcsc_amd.Plan.launch_info_q8)
    assert callable(tcsc_amd.quant_fuse_pays)
    assert tcsc_amd.XTYPE_ID == {"f32": 0, "bf16": 1}


def tiles_per_wg(M, N, cus=256):
    """decode_tiles_per_wg restated (csrc/tcsc_decode.hip)."""
    ntiles = (N + 15) // 16
    T = 4 if M > 8 else 2 if M > 4 else 1
    while T > 1 and (ntiles + T - 1) // T < cus:
        T >>= 1
    return T


def rule(M, K, N, xtype):
    """The rule of include/tcsc_gpu.h: at most 4 rows, and at most 2^23 values quantized by all workgroups together."""
    if not (1 <= M <= 4 and K >= 1 and N >= 1 and xtype in (0, 1)):
        return False
    T = tiles_per_wg(M, N)
    wgs = ((N + 15) // 16 + T - 1) // T
    return wgs * M * K <= 1 << 23


def test_quant_fuse_pays_is_0_outside_its_domain(built_lib):
    f = built_lib.tcsc_gpu_quant_fuse_pays
    for xt in (0, 1):
        assert f(0, 256, 256, xt) == 0 and f(-1, 256, 256, xt) == 0 and f(17, 256, 256, xt) == 0
        assert f(1, 0, 256, xt) == 0 and f(1, 256, 0, xt) == 0
        assert f(1, 256, 256, xt) == 1  # a small product fuses
    for xt in (-1, 2, 3, 1 << 20):
        for M in (1, 4, 16):
            assert f(M, 256, 256, xt) == 0, (M, xt)
    assert tcsc_amd.quant_fuse_pays(1, 256, 256) is True and tcsc_amd.quant_fuse_pays(1, 256, 256, "bf16") is True
    assert tcsc_amd.quant_fuse_pays(17, 256, 256, "bf16") is False and tcsc_amd.quant_fuse_pays(1, 256, 256, 2) is False
    with pytest.raises(tcsc_amd.TcscError):
        tcsc_amd.quant_fuse_pays(1, 256, 256, "fp8")


def test_quant_fuse_pays_follows_its_rule():
    for M in (1, 2, 3, 4, 5, 8, 9, 16):
        for K in (1, 256, 2560, 4096, 6912, 8192, 16384, 100003):
            for N in (1, 16, 2560, 4096, 6912, 8192, 16400, 65536):
                for xt, name in ((0, "f32"), (1, "bf16")):
                    assert tcsc_amd.quant_fuse_pays(M, K, N, name) == rule(M, K, N, xt), (M, K, N, name)
    # the measured shapes (profiles/q8_bench.json): up to M = 2 at 8192^2, up to M = 4 at the others
    for name in ("f32", "bf16"):
        assert [M for M in range(1, 17) if tcsc_amd.quant_fuse_pays(M, 8192, 8192, name)] == [1, 2]
        for K, N in ((4096, 4096), (2560, 6912), (6912, 2560)):
            assert [M for M in range(1, 17) if tcsc_amd.quant_fuse_pays(M, K, N, name)] == [1, 2, 3, 4]


@pytest.mark.parametrize("M,ldy,variant,xtype", [(4, 8, 2, 0), (4, 8, 2, 1), (-1, 8, 2, 0), (4, 8, 6, 0), (4, 8, -1, 1),
                                                 (4, 8, 2, 2), (4, 8, 2, -1), (4, -1, 2, 0)])
def test_sgemm_q8_rejects_bad_arguments_without_a_gpu(built_lib, M, ldy, variant, xtype):
    p = C.c_void_p(FAKE)
    for X, Xq, S, B, Y in ((p, p, p, p, p), (None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p),
                           (p, p, p, None, p), (p, p, p, p, None)):
        assert built_lib.tcsc_gpu_sgemm_q8(None, X, xtype, Xq, S, B, Y, M, ldy, variant, 0.2, None) == E_ARG
        assert "tcsc_gpu_sgemm_q8" in tcsc_amd.last_error()
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_sgemm_q8"):
        null_plan().sgemm_q8(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, "prelu_basic", 0.2, xtype="bf16")
    with pytest.raises(tcsc_amd.TcscError, match="fp32 or bf16"):
        null_plan().sgemm_q8(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, "prelu_basic", 0.2, xtype="int8")


def test_launch_info_q8_rejects_bad_arguments_without_a_gpu(built_lib):
    path, slices, fused = C.c_int(), C.c_int(), C.c_int()
    refs = (C.byref(path), C.byref(slices), C.byref(fused))
    f = built_lib.tcsc_gpu_launch_info_q8
    for M, xt in ((4, 0), (4, 1), (-1, 0), (4, 2), (4, -1)):
        assert f(None, M, xt, *refs) == E_ARG and "tcsc_gpu_launch_info_q8" in tcsc_amd.last_error()
    assert f(None, 4, 0, None, None, None) == E_ARG
    for dtype in ("f32", "bf16"):
        with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_launch_info_q8"):
            null_plan().launch_info_q8(4, dtype)


def test_quantize_rows_i8_bf16_rejects_bad_arguments_without_a_gpu(built_lib):
    p = C.c_void_p(FAKE)
    q = built_lib.tcsc_gpu_quantize_rows_i8_bf16
    name = "tcsc_gpu_quantize_rows_i8_bf16"
    assert q(None, 4, 8, p, p, None) == E_ARG and name in tcsc_amd.last_error()   # NULL X
    assert q(p, 4, 8, None, p, None) == E_ARG and name in tcsc_amd.last_error()   # NULL Xq
    assert q(p, 4, 8, p, None, None) == E_ARG and name in tcsc_amd.last_error()   # NULL scale
    assert q(p, -1, 8, p, p, None) == E_ARG and name in tcsc_amd.last_error()     # negative sizes
    assert q(p, 4, -1, p, p, None) == E_ARG and name in tcsc_amd.last_error()
    assert q(None, 0, 8, None, None, None) == 0                                   # M = 0: nothing to do
