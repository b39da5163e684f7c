"""The grouped int8 call: what can be checked without a device -- the four symbols, TCSC_GROUP_MAX, the
member struct and the prototypes in the header, the Python mirror, the refusals that need no live plan (answered
before any HIP call), and the fusing rule against its stated arithmetic.  The
refusals that need live plans (a member without the image, members of different K, a short ldy, a NULL dXq) are in
tests/test_gpu_group.py."""
import ctypes as C
import inspect
import os
import re

import pytest

import tcsc_amd

SYMBOLS = ("tcsc_gpu_sgemm_i8_group", "tcsc_gpu_sgemm_q8_group", "tcsc_gpu_launch_info_group",
           "tcsc_gpu_group_fuse_pays")
E_ARG = 1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tcsc_gpu.h")
# (K, member columns): the three bench shapes, then the small and ragged ones
SHAPES = ((2560, [2560, 640, 640]), (4096, [4096, 4096, 4096]), (8192, [8192, 1024, 1024]), (300, [40]), (1, [1, 1]),
          (257, [130, 15, 16, 260]), (4104, [8208, 17]))
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


def test_symbols_struct_and_prototypes(L):
    for name in SYMBOLS:
        assert name in tcsc_amd.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+TCSC_GROUP_MAX\s+4\b", text)
    assert tcsc_amd.GROUP_MAX == 4
    m = re.search(r"typedef\s+struct\s+tcsc_gpu_group_member\s*\{([^}]*)\}\s*tcsc_gpu_group_member\s*;", text)
    assert m
    fields = [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["const tcsc_gpu_plan *plan", "const float *dColScale", "const float *dB", "void *dY", "int ldy"]
    # the ctypes mirror: the same fields in the same order, pointers and one int
    mirror = tcsc_amd.group_member_t._fields_
    assert [f[0] for f in mirror] == [f.split("*")[-1].split(" ")[-1] for f in fields]
    assert [f[1] for f in mirror] == [C.c_void_p] * 4 + [C.c_int]
    assert C.sizeof(tcsc_amd.group_member_t) == 4 * C.sizeof(C.c_void_p) + 8  # the int and its padding

    def params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]

    head = ["const tcsc_gpu_group_member *members", "int count"]
    assert params("tcsc_gpu_sgemm_i8_group") == head + ["const void *dXq", "const float *dScale", "int ytype", "int M",
                                                        "void *stream"]
    assert params("tcsc_gpu_sgemm_q8_group") == head + ["const void *dX", "int xtype", "const float *dGamma",
                                                        "float eps", "void *dXq", "float *dScale", "int ytype", "int M",
                                                        "void *stream"]
    assert params("tcsc_gpu_launch_info_group") == head + ["int M", "int xtype", "int *path", "int *slices", "int *fused"]
    assert params("tcsc_gpu_group_fuse_pays") == ["int M", "int K", "const int *cols", "int count", "int xtype",
                                                  "int norm"]
    # the bindings carry one argument type per parameter
    for name in SYMBOLS:
        assert len(getattr(L, name).argtypes) == len(params(name)), name


def test_python_mirror():
    for name in ("sgemm_i8_group", "sgemm_q8_group", "launch_info_group", "group_fuse_pays"):
        assert callable(getattr(tcsc_amd, name))
    sig = inspect.signature(tcsc_amd.sgemm_i8_group).parameters
    assert list(sig) == ["plans", "Xq", "scale", "biases", "Ys", "M", "ldys", "col_scales", "stream", "ytype"]
    assert sig["ldys"].default is None and sig["col_scales"].default is None and sig["stream"].default == 0
    assert sig["ytype"].default is None
    sig = inspect.signature(tcsc_amd.sgemm_q8_group).parameters
    assert list(sig) == ["plans", "X", "Xq", "scale", "biases", "Ys", "M", "ldys", "col_scales", "norm_weight",
                         "norm_eps", "stream", "xtype", "ytype"]
    assert sig["norm_weight"].default is None and sig["norm_eps"].default is None
    sig = inspect.signature(tcsc_amd.launch_info_group).parameters
    assert list(sig) == ["plans", "M", "dtype"] and sig["dtype"].default == "f32"
    sig = inspect.signature(tcsc_amd.group_fuse_pays).parameters
    assert list(sig) == ["M", "K", "cols", "dtype", "norm"] and sig["norm"].default is False
    from tcsc_amd import nn

    assert "PackedTernaryGroup" in nn.__all__


def members(n=1, plan=None, B=P, Y=P, ldy=64):
    arr = (tcsc_amd.group_member_t * max(n, 1))()
    for k in range(n):
        arr[k].plan, arr[k].dColScale, arr[k].dB, arr[k].dY, arr[k].ldy = plan, None, B, Y, ldy
    return arr


def i8_group(L, m="one", count=1, X=P, yt=0, M=4):
    return L.tcsc_gpu_sgemm_i8_group(members() if m == "one" else m, count, X, None, yt, M, None)


def q8_group(L, m="one", count=1, X=P, xt=0, gamma=None, eps=0.0, Xq=P, S=P, yt=0, M=4):
    return L.tcsc_gpu_sgemm_q8_group(members() if m == "one" else m, count, X, xt, gamma, eps, Xq, S, yt, M, None)


def test_refusals_without_a_plan(L):
    """The order in which the entry points answer: count, NULL members, ytype, on the q8 form xtype, eps and a dGamma
    without eps (what describes the call), and then the members, first a NULL plan, named by its index.  Every call
    below violates the later checks too (its plans are NULL), so each assertion also shows that the earlier check
    answers first."""
    for call, name in ((i8_group, "tcsc_gpu_sgemm_i8_group"), (q8_group, "tcsc_gpu_sgemm_q8_group")):
        for count in (0, -1, 5, 1 << 20):
            assert "count" in _refused(L, call(L, m=None, count=count, yt=9), name)  # NULL members, bad ytype: count first
        assert "members" in _refused(L, call(L, m=None, yt=9), name)
        for yt in (2, -1):
            assert "ytype" in _refused(L, call(L, yt=yt), name)
        assert "member 0" in _refused(L, call(L), name) and "plan" in L.tcsc_gpu_last_error().decode()
    name = "tcsc_gpu_sgemm_q8_group"
    for xt in (2, -1):
        assert "xtype" in _refused(L, q8_group(L, xt=xt, eps=-1.0), name)  # ahead of eps
    assert "ytype" in _refused(L, q8_group(L, xt=2, yt=2), name)  # ytype ahead of xtype
    for eps in (-1e-6, float("inf"), float("-inf"), float("nan")):
        assert "eps" in _refused(L, q8_group(L, eps=eps), name)
    assert "dGamma" in _refused(L, q8_group(L, gamma=P, eps=0.0), name)
    assert "member 0" in _refused(L, q8_group(L, gamma=P, eps=1e-6), name)  # a norm with a gamma: on to the members
    # the index is the first offending member's: two members, of which the test can only make both NULL
    msg = _refused(L, i8_group(L, m=members(2), count=2), "tcsc_gpu_sgemm_i8_group")
    assert "member 0" in msg and "NULL plan" in msg
    path, fused = C.c_int(), C.c_int()
    slices = (C.c_int * 4)()
    name = "tcsc_gpu_launch_info_group"
    info = lambda m, count, M=4, xt=0, p=C.byref(path): L.tcsc_gpu_launch_info_group(m, count, M, xt, p, slices,
                                                                                     C.byref(fused))
    assert "count" in _refused(L, info(None, 0), name)
    assert "members" in _refused(L, info(None, 1), name)
    assert "member 0" in _refused(L, info(members(), 1), name)
    _refused(L, info(members(), 1, xt=2), name)
    _refused(L, info(members(), 1, M=-1), name)
    _refused(L, info(members(), 1, p=None), name)
    # the Python mirror passes an empty or oversized group on to the library's refusal
    with pytest.raises(tcsc_amd.TcscError, match="count"):
        tcsc_amd.launch_info_group([], 4)


def group_tiles_per_wg(M, cols, cus=256):
    """T of a grouped launch: 4 above 8 rows, 2 above 4, else 1, halved while the whole grid is below the CU count."""
    wgs = lambda T: sum(((n + 15) // 16 + T - 1) // T for n in cols)
    T = 4 if M > 8 else 2 if M > 4 else 1
    while T > 1 and wgs(T) < cus:
        T //= 2
    return T, wgs(T)


def stated_rule(M, K, cols, xt, norm):
    """§20's rule with the grouped launch's own workgroup count W; 0 with the norm and above 4 rows."""
    if norm or xt not in (0, 1) or K < 1 or not 1 <= len(cols) <= 4 or min(cols) < 1 or not 1 <= M <= 4:
        return 0
    _, W = group_tiles_per_wg(M, cols)
    return int(W * M * K <= 2 ** 23)


def test_group_fuse_pays_against_its_stated_arithmetic(L):
    seen = set()
    for K, cols in SHAPES:
        arr = (C.c_int * len(cols))(*cols)
        for xt in (0, 1, 2, -1):
            for norm in (0, 1):
                for M in range(0, 18):
                    got = L.tcsc_gpu_group_fuse_pays(M, K, arr, len(cols), xt, norm)
                    assert got == stated_rule(M, K, cols, xt, norm), (M, K, cols, xt, norm, got)
                    seen.add(got)
                    if len(cols) == 1 and not norm:
                        assert got == L.tcsc_gpu_quant_fuse_pays(M, K, cols[0], xt), (M, K, cols)
        # one member of any of the shapes' column counts is the single call's rule
        for n in cols:
            for M in range(0, 18):
                assert L.tcsc_gpu_group_fuse_pays(M, K, (C.c_int * 1)(n), 1, 1, 0) == L.tcsc_gpu_quant_fuse_pays(M, K, n, 1)
        assert tcsc_amd.group_fuse_pays(1, K, cols, "bf16") is bool(stated_rule(1, K, cols, 1, 0))
        assert tcsc_amd.group_fuse_pays(1, K, cols, "f32", norm=True) is False
    assert seen == {0, 1}
    # the T rule above 4 rows does not reach the answer (0 there), below it T = 1: W is the sum of the members' tiles
    assert group_tiles_per_wg(16, [8170, 17, 8200]) == (4, 258) and group_tiles_per_wg(8, [4090, 33, 4090]) == (2, 258)
    assert group_tiles_per_wg(16, [2560, 640, 640]) == (1, 240)
    # 240 workgroups x 4 rows x 2560 = 2.4 M values: fused; 768 x 4 x 4096 = 12.6 M: not; 768 x 2 x 4096 = 6.3 M: fused
    assert L.tcsc_gpu_group_fuse_pays(4, 2560, (C.c_int * 3)(2560, 640, 640), 3, 1, 0) == 1
    assert L.tcsc_gpu_group_fuse_pays(4, 4096, (C.c_int * 3)(4096, 4096, 4096), 3, 1, 0) == 0
    assert L.tcsc_gpu_group_fuse_pays(2, 4096, (C.c_int * 3)(4096, 4096, 4096), 3, 1, 0) == 1
    # arguments that describe no launch
    one = (C.c_int * 2)(64, 0)
    assert L.tcsc_gpu_group_fuse_pays(1, 64, one, 2, 0, 0) == 0 and L.tcsc_gpu_group_fuse_pays(1, 0, one, 1, 0, 0) == 0
    assert L.tcsc_gpu_group_fuse_pays(1, 64, one, 0, 0, 0) == 0 and L.tcsc_gpu_group_fuse_pays(1, 64, one, 5, 0, 0) == 0
    assert L.tcsc_gpu_group_fuse_pays(1, 64, None, 1, 0, 0) == 0
