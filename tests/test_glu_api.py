"""The gated FFN call: what can be checked without a device -- the four symbols, the enum and the
prototypes in the header, the Python mirror, the refusals that need no plan (answered before any HIP call), and the
fusing rule against its stated arithmetic.  The refusals that need live plans (a plan without the image, two plans
of different shapes, a NULL dG on the MFMA route) are in tests/test_gpu_glu.py."""
import ctypes as C
import inspect
import os
import re

import pytest

import tcsc_amd

SYMBOLS = ("tcsc_gpu_sgemm_i8_glu", "tcsc_gpu_sgemm_q8_glu", "tcsc_gpu_launch_info_glu", "tcsc_gpu_glu_fuse_pays")
E_ARG = 1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tcsc_gpu.h")
SHAPES = ((2560, 6912), (6912, 2560), (4096, 4096), (8192, 8192), (300, 40), (1, 1), (257, 130), (4104, 8208))
# never dereferenced: every check below answers before any HIP call
P = 0x1000


@pytest.fixture(scope="module")
def L():
    tcsc_amd.build()
    return tcsc_amd.lib()


def _refused(L, rc, name):
    assert rc == E_ARG, rc
    msg = L.tcsc_gpu_last_error().decode()
    assert name in msg, msg
    return msg


def test_symbols_enum_and_prototypes(L):
    for name in SYMBOLS:
        assert name in tcsc_amd.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert re.search(r"enum\s+tcsc_glu_act\s*\{\s*TCSC_GLU_RELU2\s*=\s*0\s*,\s*TCSC_GLU_SILU\s*=\s*1\s*\}", text)

    def params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]

    tail = ["const float *dColScaleG", "const float *dBG", "const float *dColScaleU", "const float *dBU", "float *dG",
            "void *dY", "int ytype", "int M", "int ldy", "int act", "void *stream"]
    plans = ["const tcsc_gpu_plan *gate", "const tcsc_gpu_plan *up"]
    assert params("tcsc_gpu_sgemm_i8_glu") == plans + ["const void *dXq", "const float *dScale"] + tail
    assert params("tcsc_gpu_sgemm_q8_glu") == plans + ["const void *dX", "int xtype", "const float *dGamma", "float eps",
                                                       "void *dXq", "float *dScale"] + tail
    assert params("tcsc_gpu_launch_info_glu") == plans + ["int M", "int xtype", "int *path", "int *slices", "int *fused"]
    assert params("tcsc_gpu_glu_fuse_pays") == ["int M", "int K", "int N", "int xtype", "int norm"]
    # the bindings carry one argument type per parameter
    for name in SYMBOLS:
        assert len(getattr(L, name).argtypes) == len(params(name)), name


def test_python_mirror():
    assert tcsc_amd.GLU_ACT_ID == {"relu2": 0, "silu": 1}
    for name in ("sgemm_i8_glu", "sgemm_q8_glu", "launch_info_glu", "glu_fuse_pays"):
        assert callable(getattr(tcsc_amd, name))
    sig = inspect.signature(tcsc_amd.sgemm_i8_glu).parameters
    assert list(sig)[:9] == ["gate_plan", "up_plan", "Xq", "scale", "bias_gate", "bias_up", "Y", "M", "ldy"]
    assert sig["act"].default == "relu2" and sig["G"].default is None
    assert sig["col_scale_gate"].default is None and sig["col_scale_up"].default is None
    sig = inspect.signature(tcsc_amd.sgemm_q8_glu).parameters
    assert list(sig)[:10] == ["gate_plan", "up_plan", "X", "Xq", "scale", "bias_gate", "bias_up", "Y", "M", "ldy"]
    assert sig["norm_weight"].default is None and sig["norm_eps"].default is None and sig["act"].default == "relu2"
    with pytest.raises(tcsc_amd.TcscError):
        tcsc_amd._glu_act("gelu")
    from tcsc_amd import nn

    assert {"PackedTernaryGLU", "PackedTernaryMLP"} <= set(nn.__all__)


def i8_glu(L, gate=None, up=None, X=P, bg=P, bu=P, G=None, Y=P, yt=0, M=4, ldy=64, act=0):
    return L.tcsc_gpu_sgemm_i8_glu(gate, up, X, None, None, bg, None, bu, G, Y, yt, M, ldy, act, None)


def q8_glu(L, gate=None, up=None, X=P, xt=0, gamma=None, eps=0.0, Xq=P, S=P, bg=P, bu=P, G=None, Y=P, yt=0, M=4,
           ldy=64, act=0):
    return L.tcsc_gpu_sgemm_q8_glu(gate, up, X, xt, gamma, eps, Xq, S, None, bg, None, bu, G, Y, yt, M, ldy, act, None)


def test_refusals_without_a_plan(L):
    """act and ytype out of range are answered ahead of the NULL plan, which is answered too -- for the gate and for
    the up plan (the gate's is asked first); on the q8 form also xtype, eps and a dGamma without eps."""
    for call, name in ((i8_glu, "tcsc_gpu_sgemm_i8_glu"), (q8_glu, "tcsc_gpu_sgemm_q8_glu")):
        for act in (2, -1, 7):
            assert "act" in _refused(L, call(L, act=act), name)
        for yt in (2, -1):
            assert "ytype" in _refused(L, call(L, yt=yt), name)
        assert "gate plan" in _refused(L, call(L), name)
        assert "gate plan" in _refused(L, call(L, up=P), name)  # never read: the NULL gate answers first
    name = "tcsc_gpu_sgemm_q8_glu"
    for xt in (2, -1):
        assert "xtype" in _refused(L, q8_glu(L, xt=xt), name)
    for eps in (-1e-6, float("inf"), float("-inf"), float("nan")):
        assert "eps" in _refused(L, q8_glu(L, eps=eps), name)
    assert "dGamma" in _refused(L, q8_glu(L, gamma=P, eps=0.0), name)
    assert "plan" in _refused(L, q8_glu(L, gamma=P, eps=1e-6), name)  # a norm with a gamma: on to the plans
    path, slices, fused = C.c_int(), C.c_int(), C.c_int()
    name = "tcsc_gpu_launch_info_glu"
    assert "plan" in _refused(L, L.tcsc_gpu_launch_info_glu(None, None, 4, 0, C.byref(path), C.byref(slices),
                                                            C.byref(fused)), name)
    _refused(L, L.tcsc_gpu_launch_info_glu(None, None, 4, 2, C.byref(path), C.byref(slices), C.byref(fused)), name)
    _refused(L, L.tcsc_gpu_launch_info_glu(None, None, -1, 0, C.byref(path), C.byref(slices), C.byref(fused)), name)
    _refused(L, L.tcsc_gpu_launch_info_glu(None, None, 4, 0, None, C.byref(slices), C.byref(fused)), name)


def glu_tiles_per_wg(M, H, cus=256):
    """TG of a gated launch: decode_tiles_per_wg's rule on the 2 TG image tiles of a workgroup."""
    ntiles = (H + 15) // 16
    T = 4 if M > 8 else 2
    while T > 2 and (ntiles + T // 2 - 1) // (T // 2) < cus:
        T //= 2
    return T // 2


def stated_rule(M, K, H, xt, norm):
    """§20's rule with the gated launch's own workgroup count; with the norm §22's, which is 0."""
    if norm or xt not in (0, 1) or K < 1 or H < 1 or not 1 <= M <= 4:
        return 0
    TG = glu_tiles_per_wg(M, H)
    W = ((H + 15) // 16 + TG - 1) // TG
    return int(W * M * K <= 2 ** 23)


def test_glu_fuse_pays_against_its_stated_arithmetic(L):
    seen = set()
    for K, H in SHAPES:
        for xt in (0, 1, 2, -1):
            for norm in (0, 1):
                for M in (-1, 0, 1, 2, 3, 4, 5, 8, 16, 17, 64):
                    got = L.tcsc_gpu_glu_fuse_pays(M, K, H, xt, norm)
                    assert got == stated_rule(M, K, H, xt, norm), (M, K, H, xt, norm, got)
                    seen.add(got)
                    if norm and xt in (0, 1):
                        assert got == L.tcsc_gpu_norm_fuse_pays(M, K, H, xt) == 0
        assert tcsc_amd.glu_fuse_pays(1, K, H, "bf16") is bool(stated_rule(1, K, H, 1, 0))
        assert tcsc_amd.glu_fuse_pays(1, K, H, "f32", norm=True) is False
    assert seen == {0, 1}
    # the workgroup count is the gated launch's: one column tile per workgroup up to M = 4
    assert L.tcsc_gpu_glu_fuse_pays(4, 4096, 4096, 0, 0) == 1 and L.tcsc_gpu_glu_fuse_pays(4, 8192, 8192, 0, 0) == 0
    assert L.tcsc_gpu_glu_fuse_pays(2, 8192, 8192, 1, 0) == 1
    for M in (1, 4):
        assert L.tcsc_gpu_glu_fuse_pays(M, 0, 64, 0, 0) == 0 and L.tcsc_gpu_glu_fuse_pays(M, 64, 0, 0, 0) == 0
