"""Gated and grouped int8 calls at 17 .. 64 rows: what can be checked without a device -- the six
new symbols and their prototypes in the header against the ctypes mirror, the refusals that need no live plan, the
two rules tcsc_gpu_glu_rows_pays / tcsc_gpu_group_rows_pays against the benchmark table they are fitted to (or 0
everywhere where there is none), and the Python surface.  Everything that needs a plan is in
tests/test_gpu_multi_rows.py."""
import ctypes as C
import inspect
import json
import os
import re

import pytest

import tcsc_amd

SYMBOLS = ("tcsc_gpu_plan_set_decode_rows_multi", "tcsc_gpu_plan_decode_rows_multi", "tcsc_gpu_glu_rows_pays",
           "tcsc_gpu_group_rows_pays", "tcsc_gpu_launch_info_glu_decode", "tcsc_gpu_launch_info_group_decode")
E_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tcsc_gpu.h")
BENCH = os.path.join(ROOT, "profiles", "multi_rows_bench.json")
GROUP_MAX = 4


@pytest.fixture(scope="module")
def L():
    tcsc_amd.build()
    lib = tcsc_amd.lib()
    for name in SYMBOLS:  # a library without the feature fails here, in every test of the file
        assert getattr(lib, name) is not None
    return lib


def ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def test_symbols_and_prototypes(L):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]

    assert params(SYMBOLS[0]) == ["tcsc_gpu_plan *plan", "int rows"]
    assert params(SYMBOLS[1]) == ["const tcsc_gpu_plan *plan"]
    assert params(SYMBOLS[2]) == ["int M", "int K", "int H", "int num_cus"]
    assert params(SYMBOLS[3]) == ["int M", "int K", "const int *cols", "int count", "int num_cus"]
    assert params(SYMBOLS[4]) == ["const tcsc_gpu_plan *gate", "const tcsc_gpu_plan *up", "int M", "int *row_tiles",
                                  "int *col_tiles", "long long *workgroups"]
    assert params(SYMBOLS[5]) == ["const tcsc_gpu_group_member *members", "int count", "int M", "int *row_tiles",
                                  "int *col_tiles", "long long *workgroups"]

    def ctype(p):
        if p.startswith("int *") or p.startswith("const int *"):
            return C.POINTER(C.c_int)
        if p.startswith("long long *"):
            return C.POINTER(C.c_longlong)
        if p.startswith("const tcsc_gpu_group_member *"):
            return C.POINTER(tcsc_amd.group_member_t)
        return C.c_void_p if "*" in p else C.c_int

    for name in SYMBOLS:
        assert name in tcsc_amd.EXPORTED_SYMBOLS
        assert list(getattr(L, name).argtypes) == [ctype(p) for p in params(name)], name


def test_null_plans_are_refused(L):
    for rows in (16, 40, 64, tcsc_amd.DECODE_ROWS_AUTO, 15, 65):
        assert L.tcsc_gpu_plan_set_decode_rows_multi(None, rows) == E_ARG
        assert "tcsc_gpu_plan_set_decode_rows_multi: NULL plan" in L.tcsc_gpu_last_error().decode()
    assert L.tcsc_gpu_plan_decode_rows_multi(None) == E_ARG
    assert "tcsc_gpu_plan_decode_rows_multi: NULL plan" in L.tcsc_gpu_last_error().decode()
    rt, ct, wg = C.c_int(7), C.c_int(7), C.c_longlong(7)
    assert L.tcsc_gpu_launch_info_glu_decode(None, None, 40, C.byref(rt), C.byref(ct), C.byref(wg)) == E_ARG
    assert "tcsc_gpu_launch_info_glu_decode: NULL gate plan" in L.tcsc_gpu_last_error().decode()
    members = (tcsc_amd.group_member_t * GROUP_MAX)()  # NULL plans
    for count in (1, 3, GROUP_MAX):
        assert L.tcsc_gpu_launch_info_group_decode(members, count, 40, C.byref(rt), C.byref(ct), C.byref(wg)) == E_ARG
        assert "tcsc_gpu_launch_info_group_decode: member 0: NULL plan" in L.tcsc_gpu_last_error().decode()
    for count in (0, -1, GROUP_MAX + 1):
        assert L.tcsc_gpu_launch_info_group_decode(members, count, 40, C.byref(rt), C.byref(ct), C.byref(wg)) == E_ARG
        assert "tcsc_gpu_launch_info_group_decode: count=" in L.tcsc_gpu_last_error().decode()
    assert L.tcsc_gpu_launch_info_group_decode(None, 2, 40, C.byref(rt), C.byref(ct), C.byref(wg)) == E_ARG
    assert (rt.value, ct.value, wg.value) == (7, 7, 7)


GLU_SHAPES = [(2560, 6912), (4096, 4096), (8192, 8192), (1, 1), (300, 77), (16384, 16384)]
GROUP_SHAPES = [(2560, [2560, 640, 640]), (4096, [4096] * 3), (8192, [8192, 1024, 1024]), (1, [1]), (300, [130, 17, 1]),
                (4096, [4096] * 4)]
CUS = (0, 64, 256, 304)


def test_the_rules_are_zero_outside_17_to_64_rows_and_for_bad_arguments(L):
    for M in (-1, 0, 1, 8, 15, 16, 65, 66, 128, 1 << 20):
        for cus in CUS:
            for K, H in GLU_SHAPES:
                assert L.tcsc_gpu_glu_rows_pays(M, K, H, cus) == 0, (M, K, H, cus)
            for K, cols in GROUP_SHAPES:
                assert L.tcsc_gpu_group_rows_pays(M, K, ints(cols), len(cols), cus) == 0, (M, K, cols, cus)
    for M in (17, 32, 33, 64):
        for K, H in ((0, 4096), (-5, 4096), (4096, 0), (4096, -1), (1 << 22, 4096)):
            assert L.tcsc_gpu_glu_rows_pays(M, K, H, 256) == 0
        for K in (0, -5, 1 << 22):
            assert L.tcsc_gpu_group_rows_pays(M, K, ints([4096, 4096]), 2, 256) == 0
        for cols in ([0], [4096, 0], [4096, -3, 4096]):  # a column count < 1
            assert L.tcsc_gpu_group_rows_pays(M, 4096, ints(cols), len(cols), 256) == 0
        for count in (0, -1, GROUP_MAX + 1):  # a count outside 1 .. TCSC_GROUP_MAX
            assert L.tcsc_gpu_group_rows_pays(M, 4096, ints([4096] * 5), count, 256) == 0
        assert L.tcsc_gpu_group_rows_pays(M, 4096, None, 2, 256) == 0


def test_the_rules_follow_the_measured_table(L):
    """Where profiles/multi_rows_bench.json exists, every measured point at which a rule says 1 has the one launch
    (B) below both samples of the parent (A); where it does not, nothing has been measured and both rules are 0
    over a grid of M, K and N."""
    if os.path.exists(BENCH):
        table = json.load(open(BENCH))
        cus = int(table.get("num_cus", 256))
        points = table["points"]
        assert points
        for pt in points:
            M, K = int(pt["M"]), int(pt["K"])
            if pt["call"] == "glu":
                says = L.tcsc_gpu_glu_rows_pays(M, K, int(pt["cols"][0]), cus)
            else:
                cols = [int(n) for n in pt["cols"]]
                says = L.tcsc_gpu_group_rows_pays(M, K, ints(cols), len(cols), cus)
            if says:
                assert pt["B_us"] < min(pt["A_us"]), pt
        return
    for M in range(1, 70):
        for cus in CUS:
            for K, H in GLU_SHAPES + [(2560, 2560), (6912, 2560), (64, 1 << 20)]:
                assert L.tcsc_gpu_glu_rows_pays(M, K, H, cus) == 0, (M, K, H, cus)
            for K, cols in GROUP_SHAPES:
                for count in range(1, len(cols) + 1):
                    assert L.tcsc_gpu_group_rows_pays(M, K, ints(cols), count, cus) == 0, (M, K, cols, count, cus)


def test_python_surface(L):
    for name in ("set_decode_rows_multi",):
        assert callable(getattr(tcsc_amd.Plan, name))
    assert isinstance(tcsc_amd.Plan.decode_rows_multi, property)
    assert list(inspect.signature(tcsc_amd.Plan.set_decode_rows_multi).parameters) == ["self", "rows"]
    assert list(inspect.signature(tcsc_amd.glu_rows_pays).parameters) == ["M", "K", "H", "num_cus"]
    assert list(inspect.signature(tcsc_amd.group_rows_pays).parameters) == ["M", "K", "cols", "num_cus"]
    assert list(inspect.signature(tcsc_amd.launch_info_glu_decode).parameters) == ["gate_plan", "up_plan", "M"]
    assert list(inspect.signature(tcsc_amd.launch_info_group_decode).parameters) == ["plans", "M"]
    for K, H in GLU_SHAPES:
        for M in (16, 17, 32, 33, 64, 65):
            assert tcsc_amd.glu_rows_pays(M, K, H, 256) == bool(L.tcsc_gpu_glu_rows_pays(M, K, H, 256))
            assert tcsc_amd.glu_rows_pays(M, K, H) == bool(L.tcsc_gpu_glu_rows_pays(M, K, H, 0))
    for K, cols in GROUP_SHAPES:
        for M in (16, 17, 32, 33, 64, 65):
            want = bool(L.tcsc_gpu_group_rows_pays(M, K, ints(cols), len(cols), 256))
            assert tcsc_amd.group_rows_pays(M, K, cols, 256) == want
    from tcsc_amd import nn

    for cls in (nn.PackedTernaryGLU, nn.PackedTernaryGroup):
        assert list(inspect.signature(cls.set_decode_rows).parameters) == ["self", "rows"]


def test_pinned_signatures_are_unchanged():
    from tcsc_amd import nn

    assert list(inspect.signature(tcsc_amd.sgemm_i8_group).parameters) == [
        "plans", "Xq", "scale", "biases", "Ys", "M", "ldys", "col_scales", "stream", "ytype"]
    assert list(inspect.signature(tcsc_amd.sgemm_q8_group).parameters) == [
        "plans", "X", "Xq", "scale", "biases", "Ys", "M", "ldys", "col_scales", "norm_weight", "norm_eps", "stream",
        "xtype", "ytype"]
    assert list(inspect.signature(tcsc_amd.launch_info_group).parameters) == ["plans", "M", "dtype"]
    assert list(inspect.signature(tcsc_amd.launch_info_glu).parameters) == ["gate_plan", "up_plan", "M", "dtype"]
    sig = inspect.signature(nn.PackedTernaryMLP.__init__).parameters
    assert list(sig) == ["self", "glu", "down", "decode_rows"] and sig["decode_rows"].default is None
    assert list(inspect.signature(nn.PackedTernaryGLU.__init__).parameters) == [
        "self", "Wg", "Wu", "bias_gate", "bias_up", "weight_scale_gate", "weight_scale_up", "act", "norm_weight",
        "norm_eps", "out_dtype", "device"]
    assert list(inspect.signature(nn.PackedTernaryGroup.__init__).parameters) == [
        "self", "Ws", "biases", "weight_scales", "norm_weight", "norm_eps", "out_dtype", "device"]
