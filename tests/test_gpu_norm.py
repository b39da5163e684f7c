"""RMSNorm inside the int8 call: tcsc_gpu_rmsnorm_rows, tcsc_gpu_quantize_rows_i8_norm and tcsc_gpu_sgemm_q8_norm
(k_rmsnorm_rows and the norm forms of k_quant_rows_i8 and k_decode8q).

The contract is an equality of bits, and there are two yardsticks, neither of them the fused call:
  (a) numpy (tests/norm_cases.py): the norm restated in float32, one rounded operation per step and the sum of
      squares in the pinned order; then np_quantize, the exact integer sums (held exactly by fp64: every |S| is
      asserted below 2^24) and the §21 formula act(fl(fl(fl(float32(S) * s) * c) + b)), rounded to bf16 for a bf16 Y;
  (b) the library's own rmsnorm_rows -> quantize_rows_i8 -> sgemm_i8 (the _out form) on the same plan.
Y (fp32 as uint32, bf16 as int16), the scales, Xn, r and Xq are compared as raw bits.  tests/test_norm_api.py shows
that (a)'s order differs in bits from other orders on these very rows.

Shapes are the smallest at which the kernels can go wrong: K around the group of 8, the 256-k block, the 8 waves' K
split and the 4096-element round of the 512 partials; N around the 16-column tile, and 8208 columns (513 tiles, a
ragged last workgroup); every M at which phase A changes its threads per row, and 17 and 33 for the packed MFMA
route.  Rows >= M of every 16-row X hold 3e38, whose square is inf: one stray read shows in ss."""

import numpy as np
import pytest

import norm_cases as nc
import pyoracle
import tcsc_amd
from test_gpu_q8 import (assert_same_bits, dev_f32, dev_x, image_plan, int_sums, np_quantize, packed_plan,
                         to_bf16_values)

pytestmark = pytest.mark.gpu

A = 0.2
EPS = nc.EPS
ALL_VARIANTS = pyoracle.VARIANTS + ("sparse_gemm",)
PRELU = pyoracle.PRELU_VARIANTS
KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")
MS = (1, 2, 4, 5, 8, 9, 16)
XTYPES = ("f32", "bf16")
NAME = "tcsc_gpu_sgemm_q8_norm"


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    import torch

    return torch


@pytest.fixture
def env(monkeypatch):
    """env(TCSC_QFUSE=..., ...): the knobs for plans and calls made from now on; every other knob is unset."""

    def set_env(**kw):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            if v is not None:
                monkeypatch.setenv(k, str(v))
        tcsc_amd.cache_clear()

    yield set_env
    tcsc_amd.cache_clear()


# ---- yardstick (a) ----------------------------------------------------------------------------------------------------

def formula(S, s, cs, b, variant, a=A):
    """§21: two multiplies in this order, the bias, the activation."""
    v = S.astype(np.float32) * np.asarray(s, np.float32)[:, None]
    if cs is not None:
        v = v * np.asarray(cs, np.float32)[None, :]
    v = v + np.asarray(b, np.float32)[None, :]
    assert v.dtype == np.float32
    return np.where(v < 0, np.float32(a) * v, v) if variant in PRELU else v


_cases = {}


def case(torch, o, K, N, density=0.67):
    """W, the 16 rows in both types (the bf16 rows as their widened values), gamma, column scales and a bias, and
    per type and gamma (True / False) the numpy norm, quantization and exact sums -- computed once per shape and
    left unchanged.  A test of M rows uses the first M."""
    key = (K, N, density)
    if key not in _cases:
        seed = nc.seed_of(K, N)
        Wd = o.ternary((K, N), density, seed)
        X = nc.rows_of(K, seed + 1)
        c = dict(Wd=Wd, Bf=o.uniform((N,), seed + 3), G=nc.gamma_of(K, seed + 4),
                 Cs=(np.abs(o.uniform((N,), seed + 5)) + np.float32(0.25)).astype(np.float32),
                 X={"f32": X, "bf16": to_bf16_values(torch, X)}, xn={}, r={}, q={}, s={}, S={})
        for xt in XTYPES:
            for g in (True, False):
                k = (xt, g)
                c["xn"][k], c["r"][k] = nc.np_rmsnorm(c["X"][xt], c["G"] if g else None, EPS)
                c["q"][k], c["s"][k] = np_quantize(c["xn"][k])
                c["S"][k] = int_sums(c["q"][k], Wd)
        assert c["s"][("f32", True)][2] == 0 and np.all(c["q"][("f32", True)][2] == 0)  # the zero row
        _cases[key] = c
    return _cases[key]


def y_bits(torch, Y):
    """Raw bits of a device or numpy Y: uint32 of fp32, int16 of bf16."""
    if isinstance(Y, np.ndarray):
        return np.ascontiguousarray(Y, np.float32).view(np.uint32)
    Y = Y.contiguous()
    return (Y.view(torch.int16) if Y.dtype == torch.bfloat16 else Y.view(torch.int32)).cpu().numpy()


def want_bits(torch, v, bf16):
    assert not np.isnan(v).any()
    if not bf16:
        return np.ascontiguousarray(v, np.float32).view(np.uint32).view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16).view(torch.int16).numpy()


def off_by(torch, t, offset):
    """A copy of the 1-D tensor t, `offset` elements into a 16-B aligned allocation."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[offset:offset + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


# ---- the calls --------------------------------------------------------------------------------------------------------

def call_norm(torch, plan, X, M, G, B, nc_, variant="prelu_basic", a=A, pad=3, xq=True, fused=None, cs=None, bf16=False,
              offset=0):
    """One sgemm_q8_norm into sentinel-filled Y, scale and Xq; returns (Y bits of the plan's columns, scale[:M], Xq or
    None).  `fused` True / False: launch_info_q8_norm is asserted, and that Xq kept its sentinel exactly when fused.
    `offset`: Y, the scales and Xq start that many elements into their allocations."""
    dev = X.device
    K, ldy = X.shape[1], nc_ + pad
    ydt = torch.bfloat16 if bf16 else torch.float32
    Y = off_by(torch, torch.full((M * ldy,), 7.0, dtype=ydt, device=dev), offset).view(M, ldy)
    S = off_by(torch, torch.full((max(16, M) + 1,), 5.0, device=dev), offset)
    Xq = off_by(torch, torch.full((M * K,), 0x5A, dtype=torch.int8, device=dev), offset).view(M, K) if xq else None
    info = plan.launch_info_q8_norm(M, X.dtype)
    if fused is not None:
        assert info[2] is fused and (info[0] == "decode" or not fused), info
    plan.sgemm_q8_norm(X, Xq, S, B, Y, M, ldy, G, EPS, variant, a, col_scale=cs)
    torch.cuda.synchronize()
    S = S.cpu().numpy()
    assert bool((Y[:, nc_:] == 7.0).all()), "columns beyond the plan's were written"
    assert np.all(S[M:] == 5.0), "scales beyond M were written"
    if xq:
        assert bool((Xq == 0x5A).all()) is bool(info[2]), "dXq is written exactly when the call is not fused"
    return y_bits(torch, Y[:, :nc_]), S[:M], (Xq.cpu().numpy() if xq else None)


def call_composed(torch, plan, X, M, G, B, nc_, variant="prelu_basic", a=A, cs=None, bf16=False):
    """Yardstick (b): rmsnorm_rows into an fp32 Xn, quantize_rows_i8 of Xn, sgemm_i8 (_out) on the same plan."""
    dev = X.device
    K = X.shape[1]
    Xn = torch.empty((M, K), device=dev)
    R = torch.empty(M, device=dev)
    Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
    S = torch.empty(M, device=dev)
    Y = torch.empty((M, nc_), dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    tcsc_amd.rmsnorm_rows(X, Xn, M, K, G, EPS, R)
    tcsc_amd.quantize_rows_i8(Xn, Xq, S, M, K)
    plan.sgemm_i8(Xq, S, B, Y, M, nc_, variant, a, col_scale=cs)
    torch.cuda.synchronize()
    return y_bits(torch, Y), S.cpu().numpy(), Xq.cpu().numpy(), Xn.cpu().numpy(), R.cpu().numpy()


def check(torch, plan, c, xt, M, nc_, gamma=True, cols=slice(None), variant="prelu_basic", a=A, offset=0, fused=True,
          cscale=False, bf16=False, what=""):
    """One sgemm_q8_norm call against both yardsticks, and yardstick (b)'s own steps against (a)."""
    what = f"{what} {xt} M={M} gamma={gamma} cs={cscale} bf16={bf16}"
    k = (xt, gamma)
    X = dev_x(torch, c["X"][xt], xt, M, offset)
    G = off_by(torch, dev_f32(torch, c["G"]), offset) if gamma else None
    B = dev_f32(torch, c["Bf"][cols])
    cs = c["Cs"][cols] if cscale else None
    csd = dev_f32(torch, cs) if cscale else None
    Y, S, Xq = call_norm(torch, plan, X, M, G, B, nc_, variant, a, fused=fused, cs=csd, bf16=bf16, offset=offset)
    assert_same_bits(S, c["s"][k][:M], what + " scales (a)")
    want = formula(c["S"][k][:M, cols], c["s"][k][:M], cs, c["Bf"][cols], variant, a)
    np.testing.assert_array_equal(Y, want_bits(torch, want, bf16), err_msg=what + " (a)")
    if not fused:
        np.testing.assert_array_equal(Xq, c["q"][k][:M], err_msg=what + " Xq (a)")
    Yb, Sb, qb, xnb, rb = call_composed(torch, plan, X, M, G, B, nc_, variant, a, cs=csd, bf16=bf16)
    assert_same_bits(rb, c["r"][k][:M], what + " r (a)")
    assert_same_bits(xnb, c["xn"][k][:M], what + " Xn (a)")
    np.testing.assert_array_equal(qb, c["q"][k][:M], err_msg=what + " quantizer (a)")
    assert_same_bits(S, Sb, what + " scales (b)")
    np.testing.assert_array_equal(Y, Yb, err_msg=what + " (b)")


def check_standalone(torch, c, xt, K, offset=0, what=""):
    """rmsnorm_rows and quantize_rows_i8_norm on all 16 rows (16 workgroups), with and without gamma, against (a);
    Xn, r, Xq and the scales `offset` elements into their allocations."""
    dev = torch.device("cuda:0")
    for gamma in (True, False):
        k = (xt, gamma)
        X = dev_x(torch, c["X"][xt], xt, 16, offset)
        G = off_by(torch, dev_f32(torch, c["G"]), offset) if gamma else None
        Xn = off_by(torch, torch.full((16 * K,), 7.0, device=dev), offset).view(16, K)
        R = off_by(torch, torch.full((16,), 5.0, device=dev), offset)
        tcsc_amd.rmsnorm_rows(X, Xn, 16, K, G, EPS, R)
        Xq = off_by(torch, torch.full((16 * K,), 0x5A, dtype=torch.int8, device=dev), offset).view(16, K)
        S = off_by(torch, torch.full((16,), 5.0, device=dev), offset)
        tcsc_amd.quantize_rows_i8_norm(X, Xq, S, 16, K, G, EPS)
        Xn2 = torch.full((16, K), 7.0, device=dev)
        tcsc_amd.rmsnorm_rows(X, Xn2, 16, K, G, EPS)  # no rinv
        torch.cuda.synchronize()
        w = f"{what} K={K} {xt} gamma={gamma} offset={offset}"
        assert_same_bits(R.cpu().numpy(), c["r"][k], w + " r")
        assert_same_bits(Xn.cpu().numpy(), c["xn"][k], w + " Xn")
        assert_same_bits(Xn2.cpu().numpy(), c["xn"][k], w + " Xn without rinv")
        np.testing.assert_array_equal(Xq.cpu().numpy(), c["q"][k], err_msg=w + " Xq")
        assert_same_bits(S.cpu().numpy(), c["s"][k], w + " scales")


# ---- 1. shape edges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", nc.KS)
def test_k_edges(gpu, oracle, env, K):
    torch = gpu
    N = 40
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    for xt in XTYPES:
        check_standalone(torch, c, xt, K)
        for M in MS:
            check(torch, plan, c, xt, M, N, gamma=True, cscale=M in (2, 9), bf16=M in (2, 16), what=f"K={K}")
        for M in (1, 5, 16):
            check(torch, plan, c, xt, M, N, gamma=False, what=f"K={K}")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("N", [16, 17, 40])
def test_n_edges(gpu, oracle, env, N):
    torch = gpu
    K = 300  # two blocks: six of the eight waves have none, and still take part in phase A
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    for xt in XTYPES:
        for M in MS:
            check(torch, plan, c, xt, M, N, gamma=M != 4, cscale=M == 5, bf16=M in (1, 9), what=f"N={N}")
    plan.destroy()
    W.free()


def test_a_ragged_last_workgroup(gpu, oracle, env):
    """8208 columns = 513 tiles: at M = 5, 9 and 16 a workgroup owns two tiles on a 256-CU chip and the last
    workgroup one real tile; every workgroup computes the same r and scales.  16400 columns = 1025 tiles
    (K = 260): at M = 9 and 16 a workgroup owns four (decode_tiles_per_wg(9, 16400, 256) == 4), 257 workgroups,
    the last again with one real tile."""
    torch = gpu
    env(TCSC_QFUSE="1")
    for K, N, ms in ((264, 8208, (5, 9, 16)), (260, 16400, (9, 16))):
        c = case(torch, oracle, K, N)
        W, plan = packed_plan(c["Wd"])
        for xt in XTYPES:
            for M in ms:
                check(torch, plan, c, xt, M, N, cscale=M == 9, bf16=M == 16, what=f"N={N}")
        plan.destroy()
        W.free()


@pytest.mark.parametrize("K", [256, 300])
def test_every_pointer_one_element_off_16_byte_alignment(gpu, oracle, env, K):
    """K = 256 would take the 16-B loads and stores; with X, gamma, Xn, r, Xq, the scales and Y one element off
    (4, 2 or 1 bytes) they may not be used."""
    torch = gpu
    N = 40
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    for xt in XTYPES:
        check_standalone(torch, c, xt, K, offset=1, what="unaligned")
        for knob, M in (("1", 1), ("1", 5), ("1", 16), ("0", 3)):
            env(TCSC_QFUSE=knob)
            check(torch, plan, c, xt, M, N, offset=1, fused=knob == "1", bf16=M == 5, what=f"K={K} unaligned")
    # gamma alone off, X aligned: the 16-B loads of X with scalar loads of gamma
    env(TCSC_QFUSE="1")
    for xt in XTYPES:
        for M in (1, 16):
            X = dev_x(torch, c["X"][xt], xt, M)
            G = off_by(torch, dev_f32(torch, c["G"]), 1)
            Y, S, _ = call_norm(torch, plan, X, M, G, dev_f32(torch, c["Bf"]), N, fused=True)
            k = (xt, True)
            assert_same_bits(S, c["s"][k][:M], "gamma off: scales")
            want = formula(c["S"][k][:M], c["s"][k][:M], None, c["Bf"], "prelu_basic")
            np.testing.assert_array_equal(Y, want_bits(torch, want, False), err_msg=f"gamma off {xt} M={M}")
    plan.destroy()
    W.free()


# ---- 2. variants, knobs, arguments --------------------------------------------------------------------------------------

def test_every_variant_and_slope(gpu, oracle, env):
    torch = gpu
    K, N = 333, 77
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    for xt in XTYPES:
        for M in (3, 16):
            for variant in ALL_VARIANTS:
                check(torch, plan, c, xt, M, N, variant=variant, a=0.2, cscale=True, what=variant)
            check(torch, plan, c, xt, M, N, variant="prelu_basic", a=-1.75, bf16=True, what="a=-1.75")
    plan.destroy()
    W.free()


def test_launch_info_agrees_with_what_ran_under_the_knob(gpu, oracle, env):
    """TCSC_QFUSE=0 never fuses, 1 always does on a decode route, unset follows norm_fuse_pays; what ran shows in
    dXq (written exactly when not fused), and the bits are one."""
    torch = gpu
    K, N = 333, 77
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    for xt in XTYPES:
        for M in (1, 16):
            X = dev_x(torch, c["X"][xt], xt, M)
            G, B = dev_f32(torch, c["G"]), dev_f32(torch, c["Bf"])
            got = {}
            for knob in ("1", "0", None):
                env(TCSC_QFUSE=knob)
                want = knob == "1" or (knob is None and tcsc_amd.norm_fuse_pays(M, K, N, xt))
                assert plan.launch_info_q8_norm(M, xt) == ("decode", 1, want), (knob, plan.launch_info_q8_norm(M, xt))
                assert plan.launch_info_q8_norm(M, xt)[:2] == plan.launch_info_i8(M)
                got[knob] = call_norm(torch, plan, X, M, G, B, N, fused=want)
            for knob in ("0", None):
                np.testing.assert_array_equal(got[knob][0], got["1"][0], err_msg=f"{xt} M={M} knob={knob}")
                assert_same_bits(got[knob][1], got["1"][1], f"{xt} M={M} knob={knob} scales")
            np.testing.assert_array_equal(got["0"][2], c["q"][(xt, True)][:M], err_msg="Xq of the two launches (a)")
    plan.destroy()
    W.free()


def test_arguments_on_a_live_plan(gpu, oracle, env):
    """A NULL dXq is accepted on the fused route and TCSC_E_ARG elsewhere; a bad eps or xtype, a NULL X, scale, B or
    Y, M < 0 and ldy < cols are TCSC_E_ARG with a message naming the call, and nothing is written."""
    torch = gpu
    K, N, M = 300, 40, 4
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    X = dev_x(torch, c["X"]["f32"], "f32", M)
    G, B = dev_f32(torch, c["G"]), dev_f32(torch, c["Bf"])
    env(TCSC_QFUSE="1")
    Y, S, _ = call_norm(torch, plan, X, M, G, B, N, xq=False, fused=True)
    k = ("f32", True)
    want = formula(c["S"][k][:M], c["s"][k][:M], None, c["Bf"], "prelu_basic")
    np.testing.assert_array_equal(Y, want_bits(torch, want, False), err_msg="NULL dXq, fused")
    dev = X.device
    Yd, Sd = torch.full((M, N), 7.0, device=dev), torch.full((M,), 5.0, device=dev)
    Xq = torch.full((M, K), 0x5A, dtype=torch.int8, device=dev)
    err = r"status 1\).*" + NAME
    for knob, rows in (("0", M), ("1", 17)):  # not fused: by the knob, and off the decode route
        env(TCSC_QFUSE=knob)
        Xr = dev_f32(torch, np.ones((rows, K), np.float32))
        with pytest.raises(tcsc_amd.TcscError, match=err + ".*dXq"):
            plan.sgemm_q8_norm(Xr, None, torch.empty(rows, device=dev), B, torch.empty((rows, N), device=dev), rows, N, G)
    for knob in ("1", "0"):
        env(TCSC_QFUSE=knob)
        for eps in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(tcsc_amd.TcscError, match=err + ".*eps"):
                plan.sgemm_q8_norm(X, Xq, Sd, B, Yd, M, N, G, eps)
        for xt in (2, -1):
            with pytest.raises(tcsc_amd.TcscError, match=err + ".*xtype"):
                plan.sgemm_q8_norm(X, Xq, Sd, B, Yd, M, N, G, EPS, xtype=xt)
            with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_launch_info_q8_norm"):
                plan.launch_info_q8_norm(M, xt)
        for args in ((None, Xq, Sd, B, Yd), (X, Xq, None, B, Yd), (X, Xq, Sd, None, Yd), (X, Xq, Sd, B, None)):
            with pytest.raises(tcsc_amd.TcscError, match=err):
                plan.sgemm_q8_norm(*args, M, N, G, EPS, xtype="f32")
        with pytest.raises(tcsc_amd.TcscError, match=err):
            plan.sgemm_q8_norm(X, Xq, Sd, B, Yd, M, N - 1, G)  # ldy < cols
        with pytest.raises(tcsc_amd.TcscError, match=err):
            plan.sgemm_q8_norm(X, Xq, Sd, B, Yd, -1, N, G)
        with pytest.raises(tcsc_amd.TcscError, match=err + ".*ytype"):
            plan.sgemm_q8_norm(X, Xq, Sd, B, Yd, M, N, G, EPS, ytype=2)
    torch.cuda.synchronize()
    assert bool((Yd == 7.0).all()) and bool((Sd == 5.0).all()) and bool((Xq == 0x5A).all())
    plan.destroy()
    W.free()


# ---- 3. the routes that do not fuse ---------------------------------------------------------------------------------------

def test_packed_plan_above_16_rows(gpu, oracle, env):
    """M = 17 and 33 on a packed plan: the norm form of the quantizer, k_pack8 and k_gemm8w2 -- both yardsticks."""
    torch = gpu
    K, N = 333, 77
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    dev = torch.device("cuda:0")
    for xt in XTYPES:
        for M in (17, 33):
            x = np.concatenate([nc.rows_of(K, 31000 + M)] * 3)[:M] * np.linspace(0.5, 2.0, M, dtype=np.float32)[:, None]
            x = x if xt == "f32" else to_bf16_values(torch, x)
            X = torch.from_numpy(x).to(dev).to(torch.float32 if xt == "f32" else torch.bfloat16)
            for gamma, cscale, bf16 in ((True, True, False), (False, False, True)):
                G = dev_f32(torch, c["G"]) if gamma else None
                cs = c["Cs"] if cscale else None
                csd = dev_f32(torch, cs) if cscale else None
                B = dev_f32(torch, c["Bf"])
                assert plan.launch_info_q8_norm(M, xt) == ("mfma", plan.launch_info_i8(M)[1], False)
                Y, S, Xq = call_norm(torch, plan, X, M, G, B, N, fused=False, cs=csd, bf16=bf16)
                xn, r = nc.np_rmsnorm(x, c["G"] if gamma else None, EPS)
                q, s = np_quantize(xn)
                what = f"{xt} M={M} gamma={gamma}"
                np.testing.assert_array_equal(Xq, q, err_msg=what + " Xq (a)")
                assert_same_bits(S, s, what + " scales (a)")
                want = formula(int_sums(q, c["Wd"]), s, cs, c["Bf"], "prelu_basic")
                np.testing.assert_array_equal(Y, want_bits(torch, want, bf16), err_msg=what + " (a)")
                Yb, Sb, qb, xnb, rb = call_composed(torch, plan, X, M, G, B, N, cs=csd, bf16=bf16)
                assert_same_bits(rb, r, what + " r (a)")
                assert_same_bits(xnb, xn, what + " Xn (a)")
                np.testing.assert_array_equal(Y, Yb, err_msg=what + " (b)")
                assert_same_bits(S, Sb, what + " scales (b)")
                np.testing.assert_array_equal(Xq, qb)
    plan.destroy()
    W.free()


def test_the_gather_and_the_small_m_route(gpu, oracle, env):
    """An ordinary plan that never built the images: the gather and the small-M path serve the int8 call and nothing
    fuses whatever TCSC_QFUSE says.  These routes take an fp32 Y without column scales -- yardstick (b)'s bits, and
    (a)'s quantizer -- and refuse anything else before a launch, naming the call and the path."""
    torch = gpu
    K, N = 333, 77
    c = case(torch, oracle, K, N)
    env(TCSC_QFUSE="1")
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan(W)
    plan.reserve(40)
    assert not plan.has_w2
    seen = set()
    dev = torch.device("cuda:0")
    for xt in XTYPES:
        for M in (1, 4, 16, 40):
            path, slices, fused = plan.launch_info_q8_norm(M, xt)
            assert (path, slices) == plan.launch_info_i8(M) and path != "decode" and fused is False
            seen.add(path)
            x = np.concatenate([c["X"][xt]] * 3)[:M]
            X = dev_f32(torch, x).to(torch.float32 if xt == "f32" else torch.bfloat16)
            G, B = dev_f32(torch, c["G"]), dev_f32(torch, c["Bf"])
            Y, S, Xq = call_norm(torch, plan, X, M, G, B, N, fused=False)
            q, s = np_quantize(nc.np_rmsnorm(x, c["G"], EPS)[0])
            np.testing.assert_array_equal(Xq, q, err_msg=f"{xt} M={M} Xq (a)")
            assert_same_bits(S, s, f"{xt} M={M} scales (a)")
            Yb, Sb, _, _, _ = call_composed(torch, plan, X, M, G, B, N)
            np.testing.assert_array_equal(Y, Yb, err_msg=f"{xt} M={M} on {path} (b)")
            assert_same_bits(S, Sb, f"{xt} M={M} scales (b)")
            if path in ("gather", "small"):
                Sd = torch.full((M,), 5.0, device=dev)
                XqD = torch.full((M, K), 0x5A, dtype=torch.int8, device=dev)
                for kw, Yd in ((dict(col_scale=dev_f32(torch, c["Cs"])), torch.full((M, N), 7.0, device=dev)),
                               (dict(), torch.full((M, N), 7.0, dtype=torch.bfloat16, device=dev))):
                    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*" + NAME):
                        plan.sgemm_q8_norm(X, XqD, Sd, B, Yd, M, N, G, EPS, **kw)
                    torch.cuda.synchronize()
                    assert bool((Yd == 7.0).all()) and bool((Sd == 5.0).all()) and bool((XqD == 0x5A).all())
    assert {"gather", "small"} <= seen, seen
    plan.destroy()
    W.free()


def test_ordinary_shard_and_transposed_plans_fuse(gpu, oracle, env):
    """The fused route on an ordinary plan with both images: a column shard (col_begin > 0, a ragged last tile) and
    a transposed plan."""
    torch = gpu
    K, N = 333, 77
    c = case(torch, oracle, K, N)
    c0, c1 = 5, 60
    W, plan = image_plan(env, c["Wd"], c0, c1, TCSC_QFUSE="1")
    for xt in XTYPES:
        for M in (1, 16):
            check(torch, plan, c, xt, M, c1 - c0, cols=slice(c0, c1), cscale=M == 16, bf16=M == 1, what="shard")
    plan.destroy()
    tplan = tcsc_amd.Plan.transposed(W)
    tplan.reserve(16)
    assert tplan.enable_i8() and tplan.enable_w2()
    ct = case(torch, oracle, N, K)  # rows of N values, a bias of K
    Wt = np.ascontiguousarray(c["Wd"].T)
    for xt in XTYPES:
        for M in (1, 16):
            k = (xt, True)
            X = dev_x(torch, ct["X"][xt], xt, M)
            G, B = dev_f32(torch, ct["G"]), dev_f32(torch, ct["Bf"])
            Y, S, _ = call_norm(torch, tplan, X, M, G, B, K, fused=True)
            want = formula(int_sums(ct["q"][k][:M], Wt), ct["s"][k][:M], None, ct["Bf"], "prelu_basic")
            np.testing.assert_array_equal(Y, want_bits(torch, want, False), err_msg=f"transposed {xt} M={M} (a)")
            Yb, Sb, _, _, _ = call_composed(torch, tplan, X, M, G, B, K)
            np.testing.assert_array_equal(Y, Yb, err_msg=f"transposed {xt} M={M} (b)")
            assert_same_bits(S, Sb, "transposed scales")
    tplan.destroy()
    W.free()


# ---- 4. capture -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xt", XTYPES)
def test_a_captured_call_replays_on_new_inputs(gpu, oracle, env, xt):
    """One fused call captured, replayed on two different X's: each X's bits, and the plan holds what it held."""
    torch = gpu
    K, N, M = 1000, 300, 2
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    assert plan.launch_info_q8_norm(M, xt) == ("decode", 1, True)
    dev = torch.device("cuda:0")
    held = plan.info()["device_bytes"]
    Xg = torch.zeros((M, K), dtype=torch.float32 if xt == "f32" else torch.bfloat16, device=dev)
    Sg, Yg = torch.zeros(M, device=dev), torch.empty((M, N), device=dev)
    G, Bf = dev_f32(torch, c["G"]), dev_f32(torch, c["Bf"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm_q8_norm(Xg, None, Sg, Bf, Yg, M, N, G, EPS, "prelu_basic", A, torch.cuda.current_stream().cuda_stream)
    k = (xt, True)
    for r0 in (0, 5):
        Xg.copy_(torch.from_numpy(c["X"][xt][r0:r0 + M]).to(dev))
        Yg.fill_(float("nan"))
        Sg.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rows = slice(r0, r0 + M)
        want = formula(c["S"][k][rows], c["s"][k][rows], None, c["Bf"], "prelu_basic")
        np.testing.assert_array_equal(y_bits(torch, Yg), want_bits(torch, want, False), err_msg=f"replay, rows {r0}..")
        assert_same_bits(Sg.cpu().numpy(), c["s"][k][rows], "replayed scales")
    assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()


# ---- 5. the layer -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("knob", [None, "1"])
def test_the_layer_with_a_norm(gpu, oracle, env, knob):
    """PackedTernaryLinear(norm_weight, norm_eps): the bits of Plan.sgemm_q8_norm, and close to
    torch.nn.functional.rms_norm followed by the layer without a norm.  torch sums the squares in another order, so
    its xn differs from the library's by a few ulp -- far less than one quantization step s[m] = amax / 127, but
    enough to move a value across a rounding boundary: each q[k] may differ by one step, so the integer sum by at
    most sum_k |w[k, j]|, and the output by s[m] * beta[j] * sum_k |w[k, j]| (PReLU with |a| <= 1 does not stretch
    it).  The scale itself differs by a few ulp too: at most 8 ulp of 2^-23 on |S| <= 127 sum_k |w|, another
    127 * 2^-20 of the same bound.  The state_dict round trip restores the bits of forward."""
    torch = gpu
    env(TCSC_QFUSE=knob)
    from tcsc_amd.nn import PackedTernaryLinear

    K, N = 300, 130
    c = case(torch, oracle, K, N)
    beta = 0.037
    normed = PackedTernaryLinear(c["Wd"], bias=c["Bf"], a=A, weight_scale=beta, norm_weight=c["G"], norm_eps=EPS)
    ones = PackedTernaryLinear(c["Wd"], bias=c["Bf"], a=A, weight_scale=beta, norm_eps=EPS)
    plain = PackedTernaryLinear(c["Wd"], bias=c["Bf"], a=A, weight_scale=beta)
    assert "norm_weight" in normed.state_dict() and "norm_weight" not in ones.state_dict()
    assert set(plain.state_dict()) == {"bias", "weight_scale", "w2"} and plain.norm_eps is None
    with pytest.raises(tcsc_amd.TcscError, match="norm_eps"):
        PackedTernaryLinear(c["Wd"], norm_weight=c["G"])
    absw = np.abs(c["Wd"]).sum(axis=0).astype(np.float64)
    dev = torch.device("cuda:0")
    Gd, Bd, Cd = dev_f32(torch, c["G"]), dev_f32(torch, c["Bf"]), torch.full((N,), beta, device=dev)
    for M in (1, 4, 16, 20):
        for xt in XTYPES:
            x = np.concatenate([c["X"][xt]] * 2)[:M]
            X = dev_f32(torch, x).to(torch.float32 if xt == "f32" else torch.bfloat16)
            with torch.no_grad():
                y = normed(X)
                y1 = ones(X)
                ref = plain(torch.nn.functional.rms_norm(X.float(), (K,), Gd, EPS))
                ref1 = plain(torch.nn.functional.rms_norm(X.float(), (K,), None, EPS))
            torch.cuda.synchronize()
            assert y.dtype == torch.float32 and y.shape == (M, N)
            # the layer is the call
            Yd, Sd = torch.empty((M, N), device=dev), torch.empty(M, device=dev)
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            normed.plan.sgemm_q8_norm(X, Xq, Sd, Bd, Yd, M, N, Gd, EPS, "prelu_basic", A, col_scale=Cd)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(y_bits(torch, y), y_bits(torch, Yd), err_msg=f"M={M} {xt}: the layer's bits")
            for got, want, gamma in ((y, ref, c["G"]), (y1, ref1, None)):
                s = np_quantize(nc.np_rmsnorm(x, gamma, EPS)[0])[1].astype(np.float64)
                bound = s[:, None] * beta * absw[None, :] * (1.0 + 127.0 * 2.0 ** -20)
                diff = np.abs(got.cpu().numpy().astype(np.float64) - want.cpu().numpy().astype(np.float64))
                print(f"M={M} {xt} gamma={gamma is not None}: worst diff / bound "
                      f"{np.max(diff / np.maximum(bound, 1e-300)):.3g}")
                assert np.all(diff <= bound), f"M={M} {xt}: {np.max(diff - bound)} beyond one quantization step"
    # the round trip: a layer made empty with the same norm_eps, loaded, gives forward's bits
    X = dev_f32(torch, c["X"]["f32"][:5])
    with torch.no_grad():
        y = normed(X)
    sd = normed.state_dict()
    loaded = PackedTernaryLinear.empty(K, N, a=A, norm_eps=EPS)
    loaded.load_state_dict(sd)
    assert loaded.norm_weight is not None and bool((loaded.norm_weight == normed.norm_weight).all())
    with torch.no_grad():
        y2 = loaded(X)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y_bits(torch, y2), y_bits(torch, y), err_msg="state_dict round trip")
    with pytest.raises(tcsc_amd.TcscError, match="norm_eps"):
        PackedTernaryLinear.empty(K, N, a=A).load_state_dict(sd)
    # a layer built without a norm saves and loads as before
    again = PackedTernaryLinear.empty(K, N, a=A)
    again.load_state_dict(plain.state_dict())
    assert again.norm_weight is None and again.norm_eps is None
    with torch.no_grad():
        np.testing.assert_array_equal(y_bits(torch, again(X)), y_bits(torch, plain(X)))
