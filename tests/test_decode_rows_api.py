"""int8 decode up to 64 rows: what can be checked without a device -- the new symbols and their
prototypes in the header against the ctypes mirror, the refusals that need no live plan, the rule
tcsc_gpu_decode_rows_pays as DESIGN states it, and the Python surface.  Everything that needs a plan is in
tests/test_gpu_decode_rows.py."""
import ctypes as C
import inspect
import os
import re

import pytest

import tcsc_amd

SYMBOLS = ("tcsc_gpu_plan_set_decode_rows", "tcsc_gpu_plan_decode_rows", "tcsc_gpu_decode_rows_pays",
           "tcsc_gpu_launch_info_decode")
E_ARG = 1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tcsc_gpu.h")


@pytest.fixture(scope="module")
def L():
    tcsc_amd.build()
    lib = tcsc_amd.lib()
    for name in SYMBOLS:  # a library without the feature fails here, in every test of the file
        assert getattr(lib, name) is not None
    return lib


def test_symbols_and_prototypes(L):
    raw = open(HEADER).read()
    assert re.search(r"#define\s+TCSC_DECODE_ROWS_AUTO\s+\(-1\)", raw)
    assert tcsc_amd.DECODE_ROWS_AUTO == -1
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]

    assert params(SYMBOLS[0]) == ["tcsc_gpu_plan *plan", "int rows"]
    assert params(SYMBOLS[1]) == ["const tcsc_gpu_plan *plan"]
    assert params(SYMBOLS[2]) == ["int M", "int K", "int N", "int num_cus"]
    assert params(SYMBOLS[3]) == ["const tcsc_gpu_plan *plan", "int M", "int *row_tiles", "int *col_tiles",
                                  "long long *workgroups"]

    def ctype(p):
        if p.startswith("int *"):
            return C.POINTER(C.c_int)
        if p.startswith("long long *"):
            return C.POINTER(C.c_longlong)
        return C.c_void_p if "*" in p else C.c_int

    for name in SYMBOLS:
        assert name in tcsc_amd.EXPORTED_SYMBOLS
        assert list(getattr(L, name).argtypes) == [ctype(p) for p in params(name)], name


def test_a_null_plan_is_refused(L):
    for rows in (16, 40, 64, tcsc_amd.DECODE_ROWS_AUTO, 15, 65):
        assert L.tcsc_gpu_plan_set_decode_rows(None, rows) == E_ARG
        assert "tcsc_gpu_plan_set_decode_rows: NULL plan" in L.tcsc_gpu_last_error().decode()
    assert L.tcsc_gpu_plan_decode_rows(None) == E_ARG
    assert "tcsc_gpu_plan_decode_rows: NULL plan" in L.tcsc_gpu_last_error().decode()
    rt, ct, wg = C.c_int(7), C.c_int(7), C.c_longlong(7)
    assert L.tcsc_gpu_launch_info_decode(None, 40, C.byref(rt), C.byref(ct), C.byref(wg)) == E_ARG
    assert "tcsc_gpu_launch_info_decode" in L.tcsc_gpu_last_error().decode()
    assert (rt.value, ct.value, wg.value) == (7, 7, 7)


SHAPES = [(2560, 2560), (2560, 6912), (6912, 2560), (4096, 4096), (8192, 8192), (1, 1), (300, 77), (16384, 16384),
          (4194303, 64)]


def test_the_rule_is_zero_outside_17_to_64_rows(L):
    for K, N in SHAPES:
        for cus in (0, 64, 256, 304):
            for M in (-1, 0, 1, 8, 15, 16, 65, 66, 128, 1 << 20):
                assert L.tcsc_gpu_decode_rows_pays(M, K, N, cus) == 0, (M, K, N, cus)
    for M in (17, 32, 64):  # no such launch: K >= 2^22, or nothing to compute
        for K, N in ((1 << 22, 4096), (0, 4096), (4096, 0), (-5, 4096)):
            assert L.tcsc_gpu_decode_rows_pays(M, K, N, 256) == 0


def test_the_rule_is_designs_sentence(L):
    """a row-tiled launch pays at 17 <= M <= 32 rows where K N <= 2^26, and nowhere else."""
    for K, N in SHAPES + [(8192, 8193), (8193, 8192), (1 << 13, 1 << 13), (1 << 21, 32), (1 << 21, 33)]:
        if not (1 <= K < 1 << 22):
            continue
        for cus in (0, 64, 256, 304):
            for M in range(1, 70):
                want = int(17 <= M <= 32 and K * N <= 1 << 26)
                assert L.tcsc_gpu_decode_rows_pays(M, K, N, cus) == want, (M, K, N, cus)
    # the measured shapes: 1 at every M where (B) won at all five, 0 from 33 rows on, where it lost at two of them
    for K, N in SHAPES[:5]:
        assert [L.tcsc_gpu_decode_rows_pays(M, K, N, 256) for M in (16, 17, 24, 32, 33, 48, 64)] == [0, 1, 1, 1, 0, 0, 0]


def test_python_surface():
    assert tcsc_amd.DECODE_ROWS_AUTO == -1
    for name in ("set_decode_rows", "launch_info_decode"):
        assert callable(getattr(tcsc_amd.Plan, name))
    assert isinstance(tcsc_amd.Plan.decode_rows, property)
    assert list(inspect.signature(tcsc_amd.Plan.set_decode_rows).parameters) == ["self", "rows"]
    assert list(inspect.signature(tcsc_amd.Plan.launch_info_decode).parameters) == ["self", "M"]
    assert list(inspect.signature(tcsc_amd.decode_rows_pays).parameters) == ["M", "K", "N", "num_cus"]
    from tcsc_amd import nn

    cls = nn.PackedTernaryLinear
    for f in (cls.__init__, cls.from_float, cls.empty):
        sig = inspect.signature(f).parameters
        assert list(sig)[-1] == "decode_rows" and sig["decode_rows"].default is None, f
    sig = inspect.signature(nn.PackedTernaryMLP.__init__).parameters
    assert list(sig) == ["self", "glu", "down", "decode_rows"] and sig["decode_rows"].default is None
    # nothing else changed its signature
    assert "decode_rows" not in inspect.signature(nn.PackedTernaryGLU.__init__).parameters
    assert "decode_rows" not in inspect.signature(nn.PackedTernaryGroup.__init__).parameters


def test_decode_rows_pays_in_python_is_the_librarys(L):
    for K, N in SHAPES:
        for M in (16, 17, 24, 32, 33, 48, 64, 65):
            assert tcsc_amd.decode_rows_pays(M, K, N, 256) == bool(L.tcsc_gpu_decode_rows_pays(M, K, N, 256))
            assert tcsc_amd.decode_rows_pays(M, K, N) == bool(L.tcsc_gpu_decode_rows_pays(M, K, N, 0))
