"""RMSNorm in the int8 call: what can be checked without a device -- the five symbols and their
Python mirror, the argument checks (answered before any HIP call), the fusing rule's host arithmetic, and that the
numpy restatement of the pinned summation order can be told from other orders on the rows the GPU tests use."""
import ctypes as C
import inspect

import numpy as np
import pytest

import norm_cases as nc
import tcsc_amd

SYMBOLS = ("tcsc_gpu_rmsnorm_rows", "tcsc_gpu_quantize_rows_i8_norm", "tcsc_gpu_sgemm_q8_norm",
           "tcsc_gpu_launch_info_q8_norm", "tcsc_gpu_norm_fuse_pays")
E_ARG = 1
SHAPES = ((4096, 4096), (8192, 8192), (2560, 6912), (6912, 2560), (300, 40), (1, 1), (4104, 8208))


@pytest.fixture(scope="module")
def L():
    tcsc_amd.build()
    return tcsc_amd.lib()


def test_symbols_and_mirror(L):
    for name in SYMBOLS:
        assert name in tcsc_amd.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
    for name in ("rmsnorm_rows", "quantize_rows_i8_norm", "norm_fuse_pays"):
        assert callable(getattr(tcsc_amd, name))
    for name in ("sgemm_q8_norm", "launch_info_q8_norm"):
        assert callable(getattr(tcsc_amd.Plan, name))
    sig = inspect.signature(tcsc_amd.Plan.sgemm_q8_norm).parameters
    assert sig["norm_weight"].default is None and sig["eps"].default == 1e-6
    for kw in ("variant", "a", "stream", "xtype", "col_scale", "ytype"):  # sgemm_q8's other keywords
        assert kw in sig and sig[kw].default == inspect.signature(tcsc_amd.Plan.sgemm_q8).parameters[kw].default
    sig = inspect.signature(tcsc_amd.rmsnorm_rows).parameters
    assert list(sig)[:4] == ["X", "Xn", "M", "K"] and sig["weight"].default is None and sig["eps"].default == 1e-6
    assert sig["rinv"].default is None
    sig = inspect.signature(tcsc_amd.quantize_rows_i8_norm).parameters
    assert list(sig)[:5] == ["X", "Xq", "scale", "M", "K"] and sig["weight"].default is None


def _refused(L, rc, name):
    assert rc == E_ARG, rc
    msg = L.tcsc_gpu_last_error().decode()
    assert name in msg, msg
    return msg


BAD_EPS = (0.0, -1e-6, float("inf"), float("-inf"), float("nan"))
# never dereferenced: every check below answers before any HIP call
P = 0x1000


def test_rmsnorm_rows_argument_checks(L):
    name = "tcsc_gpu_rmsnorm_rows"
    for eps in BAD_EPS:
        assert "eps" in _refused(L, L.tcsc_gpu_rmsnorm_rows(P, 0, None, eps, 4, 64, P, None, None), name)
    for K in (0, -3):
        assert "K=" in _refused(L, L.tcsc_gpu_rmsnorm_rows(P, 0, None, 1e-6, 4, K, P, None, None), name)
    for xt in (2, -1):
        assert "xtype" in _refused(L, L.tcsc_gpu_rmsnorm_rows(P, xt, None, 1e-6, 4, 64, P, None, None), name)
    assert "dXn" in _refused(L, L.tcsc_gpu_rmsnorm_rows(P, 0, None, 1e-6, 4, 64, None, None, None), name)
    assert "dXn" in _refused(L, L.tcsc_gpu_rmsnorm_rows(P, 1, None, 1e-6, 0, 64, None, None, None), name)
    _refused(L, L.tcsc_gpu_rmsnorm_rows(P, 0, None, 1e-6, -1, 64, P, None, None), name)
    assert L.tcsc_gpu_rmsnorm_rows(None, 0, None, 1e-6, 0, 64, P, None, None) == 0  # no rows: nothing to do


def test_quantize_rows_i8_norm_argument_checks(L):
    name = "tcsc_gpu_quantize_rows_i8_norm"
    for eps in BAD_EPS:
        assert "eps" in _refused(L, L.tcsc_gpu_quantize_rows_i8_norm(P, 0, None, eps, 4, 64, P, P, None), name)
    for K in (0, -3):
        assert "K=" in _refused(L, L.tcsc_gpu_quantize_rows_i8_norm(P, 1, None, 1e-6, 4, K, P, P, None), name)
    for xt in (2, -1):
        assert "xtype" in _refused(L, L.tcsc_gpu_quantize_rows_i8_norm(P, xt, None, 1e-6, 4, 64, P, P, None), name)
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        _refused(L, L.tcsc_gpu_quantize_rows_i8_norm(args[0], 0, None, 1e-6, 4, 64, args[1], args[2], None), name)
    _refused(L, L.tcsc_gpu_quantize_rows_i8_norm(P, 0, None, 1e-6, -1, 64, P, P, None), name)
    assert L.tcsc_gpu_quantize_rows_i8_norm(None, 0, None, 1e-6, 0, 64, None, None, None) == 0


def test_sgemm_q8_norm_argument_checks(L):
    """Without a device there is no plan: eps, xtype and ytype are answered ahead of the NULL plan, which is
    answered too.  (K < 1 is the plan's; the live-plan checks are in tests/test_gpu_norm.py.)"""
    name = "tcsc_gpu_sgemm_q8_norm"

    def call(plan=None, xt=0, eps=1e-6, yt=0):
        return L.tcsc_gpu_sgemm_q8_norm(plan, P, xt, None, eps, P, P, None, P, P, yt, 4, 64, 0, 0.0, None)

    for eps in BAD_EPS:
        assert "eps" in _refused(L, call(eps=eps), name)
    for xt in (2, -1):
        assert "xtype" in _refused(L, call(xt=xt), name)
    assert "ytype" in _refused(L, call(yt=2), name)
    assert "plan" in _refused(L, call(), name)
    path, slices, fused = C.c_int(), C.c_int(), C.c_int()
    _refused(L, L.tcsc_gpu_launch_info_q8_norm(None, 4, 0, C.byref(path), C.byref(slices), C.byref(fused)),
             "tcsc_gpu_launch_info_q8_norm")


def test_norm_fuse_pays_is_host_arithmetic(L):
    for K, N in SHAPES:
        for xt in (0, 1):
            for M in (0, -1, 17, 18, 64, 2048):
                assert L.tcsc_gpu_norm_fuse_pays(M, K, N, xt) == 0
            got = [L.tcsc_gpu_norm_fuse_pays(M, K, N, xt) for M in range(1, 17)]
            assert set(got) <= {0, 1}
            assert all(a >= b for a, b in zip(got, got[1:])), (K, N, xt, got)  # monotone non-increasing in M
            assert tcsc_amd.norm_fuse_pays(1, K, N, ("f32", "bf16")[xt]) is bool(got[0])
    for M in (1, 4, 16):
        assert L.tcsc_gpu_norm_fuse_pays(M, 0, 64, 0) == 0 and L.tcsc_gpu_norm_fuse_pays(M, -1, 64, 0) == 0
        assert L.tcsc_gpu_norm_fuse_pays(M, 64, 0, 0) == 0 and L.tcsc_gpu_norm_fuse_pays(M, 64, -1, 1) == 0
        assert L.tcsc_gpu_norm_fuse_pays(M, 64, 64, 2) == 0 and L.tcsc_gpu_norm_fuse_pays(M, 64, 64, -1) == 0


def test_the_pinned_order_can_be_told_from_other_orders():
    """The GPU tests compare bits against np_sumsq: a kernel that summed in another order must then differ.  On the
    tests' own rows the pinned order differs in bits from the sequential sum and from np.sum's pairwise sum, in ss
    and still in r -- at every K where more than one order exists and the sums are long enough to round apart."""
    told_seq, told_pair = [], []
    for K in nc.KS:
        X = nc.rows_of(K, nc.seed_of(K, 40) + 1)
        ss = nc.np_sumsq(X)
        assert ss.dtype == np.float32 and np.all(np.isfinite(ss)) and ss[2] == 0
        # the three orders agree to rounding: they are orders of one sum (the tiny row's squares are subnormal or
        # underflow: an absolute error of K smallest subnormals there)
        exact = np.sum(X.astype(np.float64) ** 2, axis=1)
        tiny = K * float(np.finfo(np.float32).smallest_subnormal)
        np.testing.assert_allclose(ss, exact, rtol=1e-5, atol=tiny)
        for other, told in ((nc.np_sumsq_sequential, told_seq), (nc.np_sumsq_pairwise, told_pair)):
            so = other(X)
            np.testing.assert_allclose(so, exact, rtol=1e-4, atol=tiny)
            r_differs = nc.np_rinv(ss, K).view(np.uint32) != nc.np_rinv(so, K).view(np.uint32)
            if np.any(ss.view(np.uint32) != so.view(np.uint32)) and np.any(r_differs):
                told.append(K)
    assert {255, 256, 300, 2048, 4095, 4096, 4104} <= set(told_seq), told_seq
    assert {2048, 4095, 4096, 4104} <= set(told_pair), told_pair
    # K <= 8 is one partial summed in ascending k: every order of the kernel's is the sequential one
    for K in (1, 7, 8):
        X = nc.rows_of(K, nc.seed_of(K, 40) + 1)
        np.testing.assert_array_equal(nc.np_sumsq(X).view(np.uint32), nc.np_sumsq_sequential(X).view(np.uint32))
