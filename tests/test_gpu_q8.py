"""tcsc_gpu_sgemm_q8: the quantizer fused into the int8 decode call, fp32 or bf16 X in (k_decode8q).

The contract is an equality of bits, and there are two yardsticks, neither of them the fused call:
  (a) numpy: the quantizer restated in float32 (one rounded operation per step), the exact integer sums (held
      exactly by fp64 here: every |S| is asserted below 2^24; with |q| <= 127 and K <= 4100 they stay below 2^20),
      then act(fl(fl(float32(S)) * s) + b);
  (b) the library's own quantize_rows_i8 + sgemm_i8 on the same plan.
Y and the scales are compared as uint32 bits.  Every fused case also checks that launch_info_q8 says `decode` and
fused, that a sentinel-filled dXq is untouched, that the Y columns from `cols` to ldy keep their sentinel, and that
rows >= M of a 16-row X (3e38 there) reach neither a maximum nor the scales.

Shapes are the smallest at which the kernel can go wrong: K around the 4 values of a lane's piece, the 16-byte
load, the 64-k MFMA step, the 256-k block and the 8 waves' K split (2048 k a round; 300 leaves six waves without a
block); N around the 16-column tile; 8208 columns are 513 tiles, a ragged last workgroup at two tiles a workgroup
on 256 CUs; every M at which phase A changes its threads per row (1, 2, 4, 8, 16) and one between."""

import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

A = 0.2
ALL_VARIANTS = pyoracle.VARIANTS + ("sparse_gemm",)
PRELU = pyoracle.PRELU_VARIANTS
KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")
MS = (1, 2, 4, 5, 8, 9, 16)
XTYPES = ("f32", "bf16")
BIG = 3e38


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

def np_quantize(x):
    """The quantizer restated in numpy float32, one rounded operation per step."""
    x = np.ascontiguousarray(x, np.float32)
    amax = np.max(np.abs(x), axis=1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        live = (amax > 0) & ~np.isinf(np.float32(127.0) / amax)  # a row whose 127 / amax is inf counts as a row of zeros
        scale = np.where(live, amax / np.float32(127.0), np.float32(0)).astype(np.float32)
        inv = np.where(live, np.float32(127.0) / amax, np.float32(0)).astype(np.float32)
    r = np.rint((x * inv[:, None]).astype(np.float32))
    return np.clip(r, -127, 127).astype(np.int8), scale


def int_sums(q, Wd):
    S = q.astype(np.float64) @ Wd.astype(np.float64)
    assert np.abs(S).max(initial=0) < 2 ** 24 and np.array_equal(S, np.rint(S))
    return S.astype(np.int64)


def formula(S, s, b, variant, a=A):
    v = S.astype(np.float32) * np.asarray(s, np.float32)[:, None]
    v = v + np.asarray(b, np.float32)[None, :]
    assert v.dtype == np.float32
    return np.where(v < 0, np.float32(a) * v, v) if variant in PRELU else v


def to_bf16_values(torch, x):
    """x rounded to bf16, as float32 values (what a bf16 tensor of x widens to)."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def rows_of(K, seed):
    """16 finite fp32 rows: row 0 has its maximum as the last element, row 1 a negative maximum, row 2 is all zeros,
    row 3 has equal magnitudes, row 4 is tiny, the rest are a seeded normal sample of mixed scales."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((16, K)) * rng.choice([1e-3, 1.0, 37.0], (16, 1))).astype(np.float32)
    X[0] = np.clip(X[0], -1.0, 1.0)
    X[0, K - 1] = 2.5
    X[1] = np.clip(X[1], -1.0, 1.0)
    X[1, K // 2] = -3.0
    X[2] = 0.0
    X[3] = np.where(rng.random(K) < 0.5, -0.75, 0.75).astype(np.float32)
    X[4] = X[4] * np.float32(1e-20)
    return X


_cases = {}


def case(torch, o, K, N, density=0.67):
    """W, the 16 rows in both types (the bf16 rows as their widened values), a float bias, and per type the numpy
    quantization and exact sums -- computed once per shape and left unchanged.  A test of M rows uses the first M."""
    key = (K, N, density)
    if key not in _cases:
        seed = 20000 + 3 * K + 5 * N
        Wd = o.ternary((K, N), density, seed)
        X = rows_of(K, seed + 1)
        if K == 1:  # hand-built: the single value is the row's maximum, whatever its sign or size
            X[:, 0] = [1.5, -2.25, 0.0, 3e-3, -1e-30, 127.0, -127.0, 1.0, -1.0, 0.1, 1e30, -1e-20, 5.0, -6.0, 7.0, 0.5]
        c = dict(Wd=Wd, Bf=o.uniform((N,), seed + 3), X={"f32": X, "bf16": to_bf16_values(torch, X)}, q={}, s={}, S={})
        for xt in XTYPES:
            c["q"][xt], c["s"][xt] = np_quantize(c["X"][xt])
            c["S"][xt] = int_sums(c["q"][xt], Wd)
        assert c["s"]["f32"][2] == 0 and np.all(c["q"]["f32"][2] == 0)
        _cases[key] = c
    return _cases[key]


# ---- device buffers ---------------------------------------------------------------------------------------------------

def dev_x(torch, x, xt, M, offset=0):
    """A contiguous 16-row device tensor of type xt, `offset` elements into a 16-B aligned allocation, holding the
    first M rows of x and 3e38 below them."""
    dev = torch.device("cuda:0")
    dt = torch.float32 if xt == "f32" else torch.bfloat16
    K = x.shape[1]
    buf = torch.zeros(16 * K + 16, dtype=dt, device=dev)
    v = buf[offset:offset + 16 * K].view(16, K)
    v.fill_(BIG)
    v[:M].copy_(torch.from_numpy(np.ascontiguousarray(x[:M], np.float32)).to(dev))
    assert v.is_contiguous() and v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


def dev_f32(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.device("cuda:0"))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    assert not np.isnan(want).any() and not np.isnan(got).any(), what
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def call_q8(torch, plan, X, M, B, nc, variant="prelu_basic", a=A, pad=3, xq=True, fused=None):
    """One sgemm_q8 into sentinel-filled Y, scale and Xq; returns (Y[:, :nc], scale[:M]).  `fused` True / False: the
    route is asserted, and on the fused route that Xq kept its sentinel."""
    dev = X.device
    K, ldy = X.shape[1], nc + pad
    Y = torch.full((M, ldy), 7.0, device=dev)
    S = torch.full((16,), 5.0, device=dev)
    Xq = torch.full((M, K), 0x5A, dtype=torch.int8, device=dev) if xq else None
    info = plan.launch_info_q8(M, X.dtype)
    if fused is not None:
        assert info[2] is fused and (info[0] == "decode" or not fused), info
    plan.sgemm_q8(X, Xq, S, B, Y, M, ldy, variant, a)
    torch.cuda.synchronize()
    Y, S = Y.cpu().numpy(), S.cpu().numpy()
    assert np.all(Y[:, nc:] == 7.0), "columns beyond the plan's were written"
    assert np.all(S[M:] == 5.0), "scales beyond M were written"
    if info[2] and xq:
        assert bool((Xq == 0x5A).all()), "the fused call wrote dXq"
    return Y[:, :nc], S[:M]


def call_composed(torch, plan, X, M, B, nc, variant="prelu_basic", a=A):
    """Yardstick (b): quantize_rows_i8 + sgemm_i8 on the same plan."""
    dev = X.device
    K = X.shape[1]
    Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
    S = torch.empty(M, device=dev)
    Y = torch.empty((M, nc), device=dev)
    tcsc_amd.quantize_rows_i8(X, Xq, S, M, K)
    plan.sgemm_i8(Xq, S, B, Y, M, nc, variant, a)
    torch.cuda.synchronize()
    return Y.cpu().numpy(), S.cpu().numpy(), Xq.cpu().numpy()


def check_fused(torch, plan, c, xt, M, nc, cols=slice(None), variant="prelu_basic", a=A, offset=0, what=""):
    """A fused call against both yardsticks."""
    what = f"{what} {xt} M={M}"
    X = dev_x(torch, c["X"][xt], xt, M, offset)
    B = dev_f32(torch, c["Bf"][cols])
    Y, S = call_q8(torch, plan, X, M, B, nc, variant, a, fused=True)
    assert_same_bits(S, c["s"][xt][:M], what + " scales (a)")
    assert_same_bits(Y, formula(c["S"][xt][:M, cols], c["s"][xt][:M], c["Bf"][cols], variant, a), what + " (a)")
    Yb, Sb, qb = call_composed(torch, plan, X, M, B, nc, variant, a)
    np.testing.assert_array_equal(qb, c["q"][xt][:M], err_msg=what + " quantizer")
    assert_same_bits(S, Sb, what + " scales (b)")
    assert_same_bits(Y, Yb, what + " (b)")


def packed_plan(Wd, c0=0, c1=None):
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan.packed(W, c0, W.cols if c1 is None else c1)
    plan.reserve(40)
    return W, plan


def image_plan(env, Wd, c0=0, c1=None, **knobs):
    """An ordinary plan with the int8 and the 2-bit image (made under TCSC_PATH=mfma so that a small W gets them)."""
    env(TCSC_PATH="mfma", **knobs)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan(W, c0, W.cols if c1 is None else c1)
    plan.reserve(17)
    assert plan.enable_i8() and plan.enable_w2()
    return W, plan


# ---- 1. shape edges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 2047, 2048, 2049, 4100])
def test_k_edges(gpu, oracle, env, K):
    torch = gpu
    N = 33
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    for xt in XTYPES:
        for M in MS:
            check_fused(torch, plan, c, xt, M, N, what=f"K={K}")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("N", [1, 15, 16, 17, 33])
def test_n_edges(gpu, oracle, env, N):
    torch = gpu
    K = 300  # two blocks: six of the eight waves have none, and still take part in the row maxima
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    for xt in XTYPES:
        for M in MS:
            check_fused(torch, plan, c, xt, M, N, what=f"N={N}")
    plan.destroy()
    W.free()


def test_a_ragged_last_workgroup(gpu, oracle, env):
    """8208 columns = 513 tiles: at M = 5, 9 and 16 a workgroup owns two tiles on a 256-CU chip and the last
    workgroup one real tile.  16400 columns = 1025 tiles: at M = 9 and 16 a workgroup owns four
    (decode_tiles_per_wg(9, 16400, 256) == 4), 257 workgroups, the last again with one real tile."""
    torch = gpu
    K = 260
    env(TCSC_QFUSE="1")
    for N, ms in ((8208, (5, 9, 16)), (16400, (9, 16))):
        c = case(torch, oracle, K, N)
        W, plan = packed_plan(c["Wd"])
        for xt in XTYPES:
            for M in ms:
                check_fused(torch, plan, c, xt, M, N, what=f"N={N}")
        plan.destroy()
        W.free()


@pytest.mark.parametrize("K", [256, 300])
def test_x_one_element_off_16_byte_alignment(gpu, oracle, env, K):
    """K = 256 would take the 16-B loads; 4 bytes (fp32) or 2 bytes (bf16) off they may not be used."""
    torch = gpu
    N = 33
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    for xt in XTYPES:
        for M in (1, 5, 16):
            check_fused(torch, plan, c, xt, M, N, offset=1, what=f"K={K} unaligned")
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
                check_fused(torch, plan, c, xt, M, N, variant=variant, a=0.2, what=variant)
            check_fused(torch, plan, c, xt, M, N, variant="prelu_basic", a=-1.75, what="a=-1.75")
    plan.destroy()
    W.free()


def test_the_knob_and_the_rule_give_the_same_bits(gpu, oracle, env):
    """TCSC_QFUSE=0 never fuses, 1 always does on a decode route, unset follows quant_fuse_pays; the bits are one."""
    torch = gpu
    K, N = 333, 77
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    for xt in XTYPES:
        for M in (1, 16):
            X = dev_x(torch, c["X"][xt], xt, M)
            B = dev_f32(torch, c["Bf"])
            got = {}
            for knob in ("1", "0", None):
                env(TCSC_QFUSE=knob)
                want = knob == "1" or (knob is None and tcsc_amd.quant_fuse_pays(M, K, N, xt))
                assert plan.launch_info_q8(M, xt) == ("decode", 1, want), (knob, plan.launch_info_q8(M, xt))
                got[knob] = call_q8(torch, plan, X, M, B, N, fused=want)
            for knob in ("0", None):
                assert_same_bits(got[knob][0], got["1"][0], f"{xt} M={M} knob={knob}")
                assert_same_bits(got[knob][1], got["1"][1], f"{xt} M={M} knob={knob} scales")
            assert_same_bits(got["0"][0], formula(c["S"][xt][:M], c["s"][xt][:M], c["Bf"], "prelu_basic"), "(a)")
    plan.destroy()
    W.free()


def test_arguments_on_a_live_plan(gpu, oracle, env):
    """A NULL dXq is accepted on the fused route and TCSC_E_ARG elsewhere; a NULL X, scale, B or Y, an xtype other
    than 0 or 1, M < 0 and ldy < cols are TCSC_E_ARG with a message naming the call, and nothing is written."""
    torch = gpu
    K, N, M = 300, 33, 4
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    X = dev_x(torch, c["X"]["f32"], "f32", M)
    B = dev_f32(torch, c["Bf"])
    env(TCSC_QFUSE="1")
    Y, S = call_q8(torch, plan, X, M, B, N, xq=False, fused=True)
    assert_same_bits(Y, formula(c["S"]["f32"][:M], c["s"]["f32"][:M], c["Bf"], "prelu_basic"), "NULL dXq, fused")
    dev = X.device
    Yd, Sd = torch.full((M, N), 7.0, device=dev), torch.full((M,), 5.0, device=dev)
    Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
    err = r"status 1\).*tcsc_gpu_sgemm_q8"
    for knob, rows in (("0", M), ("1", 17)):  # not fused: by the knob, and off the decode route
        env(TCSC_QFUSE=knob)
        Xr = dev_f32(torch, np.ones((rows, K), np.float32))
        with pytest.raises(tcsc_amd.TcscError, match=err + ".*dXq"):
            plan.sgemm_q8(Xr, None, torch.empty(rows, device=dev), B, torch.empty((rows, N), device=dev), rows, N)
    env(TCSC_QFUSE="1")
    for args in ((None, Xq, Sd, B, Yd), (X, Xq, None, B, Yd), (X, Xq, Sd, None, Yd), (X, Xq, Sd, B, None)):
        with pytest.raises(tcsc_amd.TcscError, match=err):
            plan.sgemm_q8(*args, M, N, xtype="f32")
    with pytest.raises(tcsc_amd.TcscError, match=err):
        plan.sgemm_q8(X, Xq, Sd, B, Yd, M, N - 1)  # ldy < cols
    with pytest.raises(tcsc_amd.TcscError, match=err):
        plan.sgemm_q8(X, Xq, Sd, B, Yd, -1, N)
    for xt in (2, -1):
        with pytest.raises(tcsc_amd.TcscError, match=err):
            plan.sgemm_q8(X, Xq, Sd, B, Yd, M, N, xtype=xt)
        with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_launch_info_q8"):
            plan.launch_info_q8(M, xt)
    torch.cuda.synchronize()
    assert bool((Yd == 7.0).all()) and bool((Sd == 5.0).all())
    plan.destroy()
    W.free()


# ---- 3. the routes that do not fuse ---------------------------------------------------------------------------------------

def test_packed_plan_above_16_rows(gpu, oracle, env):
    """M = 17 and 40 on a packed plan: the quantizer, k_pack8 and k_gemm8w2 -- yardstick (b)'s bits and (a)'s."""
    torch = gpu
    K, N = 333, 77
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    dev = torch.device("cuda:0")
    for xt in XTYPES:
        for M in (17, 40):
            x = rows_of(K, 21000 + M)
            x = np.concatenate([x] * 3)[:M] * np.linspace(0.5, 2.0, M, dtype=np.float32)[:, None]
            x = x if xt == "f32" else to_bf16_values(torch, x)
            X = torch.from_numpy(x).to(dev).to(torch.float32 if xt == "f32" else torch.bfloat16)
            B = dev_f32(torch, c["Bf"])
            assert plan.launch_info_q8(M, xt) == ("mfma", plan.launch_info_i8(M)[1], False)
            Y = torch.full((M, N + 3), 7.0, device=dev)
            S = torch.empty(M, device=dev)
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            plan.sgemm_q8(X, Xq, S, B, Y, M, N + 3)
            Yb, Sb, qb = call_composed(torch, plan, X, M, B, N)
            Y = Y.cpu().numpy()
            assert np.all(Y[:, N:] == 7.0)
            assert_same_bits(Y[:, :N], Yb, f"{xt} M={M} (b)")
            assert_same_bits(S.cpu().numpy(), Sb, f"{xt} M={M} scales (b)")
            np.testing.assert_array_equal(Xq.cpu().numpy(), qb)
            q, s = np_quantize(x)
            np.testing.assert_array_equal(qb, q)
            assert_same_bits(Yb, formula(int_sums(q, c["Wd"]), s, c["Bf"], "prelu_basic"), f"{xt} M={M} (a)")
    plan.destroy()
    W.free()


def test_a_plan_without_the_2_bit_image(gpu, oracle, env):
    """An ordinary plan that never built the images: the gather and the small-M path serve the int8 call, nothing
    fuses whatever TCSC_QFUSE says, and the call equals yardstick (b)."""
    torch = gpu
    K, N = 333, 77
    c = case(torch, oracle, K, N)
    env(TCSC_QFUSE="1")
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan(W)
    plan.reserve(40)
    assert not plan.has_w2
    seen = set()
    for xt in XTYPES:
        for M in (1, 4, 16, 40):
            path, slices, fused = plan.launch_info_q8(M, xt)
            assert (path, slices) == plan.launch_info_i8(M) and path != "decode" and fused is False
            seen.add(path)
            B = dev_f32(torch, c["Bf"])
            if M <= 16:
                X = dev_x(torch, c["X"][xt], xt, M)
                Y, S = call_q8(torch, plan, X, M, B, N, fused=False)
            else:
                dev = B.device
                X = dev_f32(torch, np.concatenate([c["X"]["bf16"]] * 3)[:M]).to(torch.float32 if xt == "f32" else torch.bfloat16)
                Yd, Sd = torch.empty((M, N), device=dev), torch.empty(M, device=dev)
                plan.sgemm_q8(X, torch.empty((M, K), dtype=torch.int8, device=dev), Sd, B, Yd, M, N)
                torch.cuda.synchronize()
                Y, S = Yd.cpu().numpy(), Sd.cpu().numpy()
            Yb, Sb, _ = call_composed(torch, plan, X, M, B, N)
            assert_same_bits(Y, Yb, f"{xt} M={M} on {path}")
            assert_same_bits(S, Sb, f"{xt} M={M} scales")
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
            check_fused(torch, plan, c, xt, M, c1 - c0, cols=slice(c0, c1), what="shard")
    plan.destroy()
    tplan = tcsc_amd.Plan.transposed(W)
    tplan.reserve(16)
    assert tplan.enable_i8() and tplan.enable_w2()
    ct = case(torch, oracle, N, K)  # rows of N values, a bias of K
    Wt = np.ascontiguousarray(c["Wd"].T)
    for xt in XTYPES:
        for M in (1, 16):
            X = dev_x(torch, ct["X"][xt], xt, M)
            B = dev_f32(torch, ct["Bf"])
            Y, S = call_q8(torch, tplan, X, M, B, K, fused=True)
            want = formula(int_sums(ct["q"][xt][:M], Wt), ct["s"][xt][:M], ct["Bf"], "prelu_basic")
            assert_same_bits(Y, want, f"transposed {xt} M={M} (a)")
            Yb, Sb, _ = call_composed(torch, tplan, X, M, B, K)
            assert_same_bits(Y, Yb, f"transposed {xt} M={M} (b)")
            assert_same_bits(S, Sb, "transposed scales")
    tplan.destroy()
    W.free()


# ---- 4. the bf16 quantizer ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 7, 8, 300, 2048])
def test_the_bf16_quantizer_equals_the_fp32_one_on_the_widened_rows(gpu, oracle, env, K):
    torch = gpu
    env()
    c = case(torch, oracle, K, 33)
    dev = torch.device("cuda:0")
    for offset in (0, 1):
        Xb = dev_x(torch, c["X"]["bf16"], "bf16", 16, offset)
        Xf = Xb.to(torch.float32).contiguous()
        out = []
        for X in (Xb, Xf):
            q = torch.full((16, K), 0x5A, dtype=torch.int8, device=dev)
            s = torch.full((16,), 5.0, device=dev)
            tcsc_amd.quantize_rows_i8(X, q, s, 16, K)
            torch.cuda.synchronize()
            out.append((q.cpu().numpy(), s.cpu().numpy()))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        assert_same_bits(out[0][1], out[1][1], "scales")
        np.testing.assert_array_equal(out[0][0], c["q"]["bf16"])
        assert_same_bits(out[0][1], c["s"]["bf16"], "scales (a)")


# ---- 5. capture -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xt", XTYPES)
def test_a_captured_call_replays_on_new_inputs(gpu, oracle, env, xt):
    """One fused call captured, replayed on two different X's: each X's bits, and the plan holds what it held."""
    torch = gpu
    K, N, M = 1000, 300, 2
    c = case(torch, oracle, K, N)
    W, plan = packed_plan(c["Wd"])
    env(TCSC_QFUSE="1")
    assert plan.launch_info_q8(M, xt) == ("decode", 1, True)
    dev = torch.device("cuda:0")
    held = plan.info()["device_bytes"]
    Xg = torch.zeros((M, K), dtype=torch.float32 if xt == "f32" else torch.bfloat16, device=dev)
    Sg, Yg, Bf = torch.zeros(M, device=dev), torch.empty((M, N), device=dev), dev_f32(torch, c["Bf"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm_q8(Xg, None, Sg, Bf, Yg, M, N, "prelu_basic", A, torch.cuda.current_stream().cuda_stream)
    for r0 in (0, 5):
        Xg.copy_(torch.from_numpy(c["X"][xt][r0:r0 + M]).to(dev))
        Yg.fill_(float("nan"))
        Sg.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rows = slice(r0, r0 + M)
        assert_same_bits(Yg.cpu().numpy(), formula(c["S"][xt][rows], c["s"][xt][rows], c["Bf"], "prelu_basic"),
                         f"replay with rows {r0}..")
        assert_same_bits(Sg.cpu().numpy(), c["s"][xt][rows], "replayed scales")
    assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()


# ---- 6. the layers ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("knob", [None, "1"])
def test_layers_take_bf16_and_keep_their_fp32_bits(gpu, oracle, env, knob):
    torch = gpu
    env(TCSC_QFUSE=knob)
    from tcsc_amd.nn import PackedTernaryLinear, TernaryLinear

    K, N = 300, 130
    c = case(torch, oracle, K, N)
    packed = PackedTernaryLinear(c["Wd"], bias=c["Bf"], a=A)
    packed.reserve(20)
    plain = TernaryLinear(c["Wd"], bias=c["Bf"], a=A)
    plain.reserve(20, int8=True, decode=True)
    gather = TernaryLinear(c["Wd"], bias=c["Bf"], a=A)  # no images: the gather or the small-M path
    for M in (1, 4, 16, 20):
        xb = np.concatenate([c["X"]["bf16"]] * 2)[:M]
        Xb = dev_f32(torch, xb).to(torch.bfloat16)
        Xf = Xb.float()
        q, s = np_quantize(xb)
        want = formula(int_sums(q, c["Wd"]), s, c["Bf"], "prelu_basic")
        with torch.no_grad():
            for name, f in (("packed", packed.forward), ("plain", plain.forward_int8), ("gather", gather.forward_int8)):
                yb, yf = f(Xb), f(Xf)
                torch.cuda.synchronize()
                assert yb.dtype == torch.float32 and yb.shape == (M, N)
                assert_same_bits(yb.cpu().numpy(), yf.cpu().numpy(), f"{name} M={M}: bf16 x against x.float()")
                exact = name == "packed" or (name == "plain" and plain.plan.launch_info_i8(M)[0] in ("decode", "mfma"))
                if exact:  # integer sums on these routes: yardstick (a) too
                    assert_same_bits(yf.cpu().numpy(), want, f"{name} M={M} (a)")
        # fp32 x: yardstick (b) on the layers' own plans
        B = dev_f32(torch, c["Bf"])
        for name, layer, f in (("packed", packed, packed.forward), ("plain", plain, plain.forward_int8),
                               ("gather", gather, gather.forward_int8)):
            with torch.no_grad():
                y = f(Xf)
            Yb, _, _ = call_composed(torch, layer.plan, Xf, M, B, N, "prelu_basic", A)
            assert_same_bits(y.cpu().numpy(), Yb, f"{name} M={M} fp32 (b)")
