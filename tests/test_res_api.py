"""The residual add in the int8 epilogue: what can be checked without a device -- the two symbols and
their prototypes in the header against the ctypes mirror, the refusals that need no live plan (answered before any
HIP call) and the order they answer in, and that the three Plan methods build the call they built before when no
residual is given.  The refusals that need a live plan (ldr < cols, dR == dY with unequal pitches, the gather and
small-M routes) are in tests/test_gpu_res.py."""
import ctypes as C
import inspect
import os
import re

import pytest

import tcsc_amd

SYMBOLS = ("tcsc_gpu_sgemm_i8_res", "tcsc_gpu_sgemm_q8_res")
E_ARG = 1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tcsc_gpu.h")
# never dereferenced: every check below answers before any HIP call
P = 0x1000


@pytest.fixture(scope="module")
def L():
    tcsc_amd.build()
    lib = tcsc_amd.lib()
    for name in SYMBOLS:  # a library without the feature fails here, in every test of the file
        assert getattr(lib, name) is not None
    return lib


def _refused(L, rc, name):
    assert rc == E_ARG, rc
    msg = L.tcsc_gpu_last_error().decode()
    assert name in msg, msg
    return msg


def test_symbols_and_prototypes(L):
    for name in SYMBOLS:
        assert name in tcsc_amd.EXPORTED_SYMBOLS
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]

    tail = ["const float *dColScale", "const float *dB", "const void *dR", "int ldr", "void *dY", "int ytype", "int M",
            "int ldy", "void *stream"]
    assert params("tcsc_gpu_sgemm_i8_res") == ["const tcsc_gpu_plan *plan", "const void *dXq", "const float *dScale"] + tail
    assert params("tcsc_gpu_sgemm_q8_res") == ["const tcsc_gpu_plan *plan", "const void *dX", "int xtype",
                                               "const float *dGamma", "float eps", "void *dXq", "float *dScale"] + tail

    # the mirror: a pointer is c_void_p, an int c_int, a float c_float, parameter by parameter
    def ctype(p):
        return C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split(" ")[0]]

    for name in SYMBOLS:
        assert list(getattr(L, name).argtypes) == [ctype(p) for p in params(name)], name


def test_python_mirror():
    for meth in ("sgemm_i8", "sgemm_q8", "sgemm_q8_norm"):
        sig = inspect.signature(getattr(tcsc_amd.Plan, meth)).parameters
        assert list(sig)[-2:] == ["residual", "ldr"], meth
        assert sig["residual"].default is None and sig["ldr"].default is None
    from tcsc_amd import nn

    for cls in (nn.PackedTernaryLinear, nn.PackedTernaryMLP):
        sig = inspect.signature(cls.forward).parameters
        assert list(sig) == ["self", "x", "residual", "inplace"]
        assert sig["residual"].default is None and sig["inplace"].default is False


def i8_res(L, plan=None, B=P, R=P, ldr=64, Y=P, yt=0, M=4, ldy=64):
    return L.tcsc_gpu_sgemm_i8_res(plan, P, None, None, B, R, ldr, Y, yt, M, ldy, None)


def q8_res(L, plan=None, xt=0, gamma=None, eps=0.0, B=P, R=P, ldr=64, Y=P, yt=0, M=4, ldy=64):
    return L.tcsc_gpu_sgemm_q8_res(plan, P, xt, gamma, eps, P, P, None, B, R, ldr, Y, yt, M, ldy, None)


def test_refusals_without_a_plan(L):
    """The order the entry points answer in: on the q8 form the xtype, a dGamma without eps and the eps itself (what
    describes the call), then on both the ytype and the NULL plan.  Every call below has a NULL plan, most a NULL
    dR, dY or dB too, so each assertion also shows that the earlier check answers first."""
    for call, name in ((i8_res, SYMBOLS[0]), (q8_res, SYMBOLS[1])):
        for yt in (2, -1):
            assert "ytype" in _refused(L, call(L, yt=yt, R=None, Y=None, B=None), name)
        for kw in ({}, dict(R=None), dict(Y=None), dict(B=None), dict(ldr=-1), dict(R=P, Y=P, ldr=64, ldy=68)):
            assert "NULL plan" in _refused(L, call(L, **kw), name), kw
    name = SYMBOLS[1]
    for xt in (2, -1):
        assert "xtype" in _refused(L, q8_res(L, xt=xt, gamma=P, eps=0.0, yt=9), name)  # ahead of dGamma, eps and ytype
    assert "dGamma" in _refused(L, q8_res(L, gamma=P, eps=0.0, yt=9), name)  # ahead of the ytype
    for eps in (-1e-6, float("inf"), float("-inf"), float("nan")):
        assert "eps" in _refused(L, q8_res(L, eps=eps, yt=9), name)
    assert "ytype" in _refused(L, q8_res(L, gamma=P, eps=1e-6, yt=9), name)  # a norm with a gamma: on to the ytype
    assert "NULL plan" in _refused(L, q8_res(L, gamma=P, eps=1e-6), name)
    assert "NULL plan" in _refused(L, q8_res(L, eps=0.0), name)  # eps == 0 with a NULL dGamma: no norm, no complaint


class _Recorder:
    """Stands in for the loaded library: records the one call a Plan method makes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)))
            return 0

        return f


def test_no_residual_is_the_call_as_it_was(L, monkeypatch):
    """residual=None on the three Plan methods: the entry point and the argument list of the parent commit; with a
    residual the new entry point, ldr defaulting to ldy."""
    rec = _Recorder()
    monkeypatch.setattr(tcsc_amd, "lib", lambda: rec)
    plan = tcsc_amd.Plan.__new__(tcsc_amd.Plan)
    plan.handle = C.c_void_p(0x10)
    X, Xq, S, B, Y, G, Cs, R = 0x100, 0x200, 0x300, 0x400, 0x500, 0x600, 0x700, 0x800
    h = 0x10
    plan.sgemm_i8(Xq, S, B, Y, 4, 64, "prelu_basic", 0.25, 7, col_scale=Cs, ytype="bf16")
    plan.sgemm_q8(X, Xq, S, B, Y, 4, 64, "basic", 0.0, 7, xtype="bf16", col_scale=Cs, ytype="bf16")
    plan.sgemm_q8_norm(X, Xq, S, B, Y, 4, 64, G, 1e-5, "prelu_basic", 0.25, 7, xtype="f32", col_scale=None, ytype="f32")
    eps = C.c_float(1e-5).value
    assert [c[0] for c in rec.calls] == ["tcsc_gpu_sgemm_i8_out", "tcsc_gpu_sgemm_q8_out", "tcsc_gpu_sgemm_q8_norm"]
    assert rec.calls[0][1] == (h, Xq, S, Cs, B, Y, 1, 4, 64, 2, 0.25, 7)
    assert rec.calls[1][1] == (h, X, 1, Xq, S, Cs, B, Y, 1, 4, 64, 0, 0.0, 7)
    got = rec.calls[2][1]
    assert got[:4] == (h, X, 0, G) and C.c_float(got[4]).value == eps and got[5:] == (Xq, S, None, B, Y, 0, 4, 64, 2, 0.25, 7)
    del rec.calls[:]
    plan.sgemm_i8(Xq, S, B, Y, 4, 64, "basic", 0.0, 7, col_scale=Cs, ytype="bf16", residual=R)
    plan.sgemm_q8(X, Xq, S, B, Y, 4, 64, "basic", 0.0, 7, xtype="bf16", col_scale=Cs, ytype="bf16", residual=R, ldr=68)
    plan.sgemm_q8_norm(X, Xq, S, B, Y, 4, 64, G, 1e-5, "basic", 0.0, 7, xtype="f32", ytype="f32", residual=Y)
    assert [c[0] for c in rec.calls] == ["tcsc_gpu_sgemm_i8_res", "tcsc_gpu_sgemm_q8_res", "tcsc_gpu_sgemm_q8_res"]
    assert rec.calls[0][1] == (h, Xq, S, Cs, B, R, 64, Y, 1, 4, 64, 7)
    assert rec.calls[1][1] == (h, X, 1, None, 0.0, Xq, S, Cs, B, R, 68, Y, 1, 4, 64, 7)
    got = rec.calls[2][1]
    assert got[:4] == (h, X, 0, G) and C.c_float(got[4]).value == eps and got[5:] == (Xq, S, None, B, Y, 64, Y, 0, 4, 64, 7)
    # a residual goes with 'basic' alone
    for variant in ("prelu_basic", "sparse_gemm"):
        with pytest.raises(tcsc_amd.TcscError, match="basic"):
            plan.sgemm_i8(Xq, S, B, Y, 4, 64, variant, 0.0, 7, residual=R)
