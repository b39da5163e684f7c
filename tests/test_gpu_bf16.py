"""tcsc_gpu_sgemm_bf16: bf16 activations on every path.

X is made on the host as bf16 bit patterns of values already representable
and handed to the device as a torch.bfloat16 tensor.  The yardsticks are the
fp32 call on the widened X (same plan, same path, same K split: equal bits),
numpy on integer inputs (exact), the fp64 oracle with the library's usual
2^-20 (|b| + sum |x|) bar, and the gather for the rows the MFMA path cannot
carry -- never the bf16 call itself.

Why the MFMA bits equal the fp32 call's: on a widened bf16 x the three-part
split is h = x, m = l = 0, so the three-part GEMM adds two all-zero parts per
64-k block to the one-part GEMM's sums, in the same order of blocks;
acc + 0 = acc, and the accumulators start at +0, so no -0 arises.
"""
import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

A = 0.25  # exact on integers


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    import torch

    return torch


@pytest.fixture
def env(monkeypatch):
    """env(TCSC_PATH=..., TCSC_SLICES=...): the knobs for plans and calls made from now on."""

    def set_env(**kw):
        for k in ("TCSC_PATH", "TCSC_SLICES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            if v is not None:
                monkeypatch.setenv(k, str(v))
        tcsc_amd.cache_clear()

    yield set_env
    tcsc_amd.cache_clear()


def bf16_bits(x):
    """bf16 bit patterns (truncation) of fp32 values."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def widen(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def dev_bf16(torch, bits, offset=0):
    """A contiguous torch.bfloat16 device tensor with these bits, starting `offset` elements into its allocation."""
    dev = torch.device("cuda:0")
    buf = torch.zeros(bits.size + 16, dtype=torch.bfloat16, device=dev)
    v = buf[offset:offset + bits.size].view(*bits.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(dev))
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + 2 * offset
    return v


def dev_f32(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.device("cuda:0"))


def call(torch, plan, X, B, M, nc, variant, bf16, ldy=None, a=A):
    """One launch into a sentinel-filled Y; the plan's columns of it, the sentinel columns checked."""
    ldy = ldy or nc
    Y = torch.full((M, ldy), 7.0, device=X.device)
    (plan.sgemm_bf16 if bf16 else plan.sgemm)(X, B, Y, M, ldy, variant, a)
    torch.cuda.synchronize()
    Y = Y.cpu().numpy()
    assert np.all(Y[:, nc:] == 7.0), "columns beyond the plan's were written"
    return Y[:, :nc]


def assert_same_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN masks differ"
    assert np.array_equal(got[~nan], want[~nan]), f"{what}: values differ"
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32), err_msg=what)


_cases = {}


def int_case(o, M, K, N, density):
    """Integer inputs exact in bf16 (|x| <= 128), integer bias, and the exact results (computed once)."""
    key = (M, K, N, density)
    if key not in _cases:
        seed = 7000 + M + 3 * K + 5 * N
        Wd = o.ternary((K, N), density, seed)
        X = o.integers((M, K), seed + 1, rng=128)
        B = o.integers((N,), seed + 2)
        assert np.array_equal(widen(bf16_bits(X)), X) and np.abs(X).max() <= 128
        # fp64 holds these integer sums exactly (K <= 4112: below 2^24), so this is the int64 result
        lin64 = (X.astype(np.float64) @ Wd.astype(np.float64) + B.astype(np.float64)).astype(np.int64)
        assert np.abs(lin64).max() < 2 ** 24
        lin = lin64.astype(np.float32)
        _cases[key] = dict(Wd=Wd, X=X, B=B, lin=lin, act=np.where(lin < 0, np.float32(A) * lin, lin))
    return _cases[key]


def float_case(o, M, K, N):
    """bf16 truncations of uniform values (their sums round, so equal bits mean an equal order of adds) and a
    float bias."""
    return bf16_bits(o.uniform((M, K), 7500 + M + K)), o.uniform((N,), 7501 + N + K)


def exact(case, variant):
    return case["act"] if variant in pyoracle.PRELU_VARIANTS else case["lin"]


# (M, K, N, density, TCSC_PATH, the path both calls must report)
# K = 144: a multiple of 16 past one 128-k tile -- the vector transpose's second k tile is mostly past K (its load
# and store guards), with a ragged second row tile.  K = 4112: a multiple of 16 past 4096 -- the small-M vector
# staging takes a second pass, on clamped addresses (small_m_fits(4, 4112): 131,712 bytes).
GATHER = [(70, 96, 80, 0.1, "gather", "gather"), (70, 101, 80, 0.1, "gather", "gather"),
          (70, 144, 80, 0.1, "gather", "gather")]
SMALL = [(M, K, 130, 0.1, None, "small") for M in (1, 3, 4) for K in (96, 101)] + \
        [(M, 4112, 130, 0.1, None, "small") for M in (1, 4)]
MFMA = [(200, 700, 300, 0.5, "mfma", "mfma"), (200, 701, 300, 0.5, "mfma", "mfma"),
        (40, 1100, 300, 0.5, "mfma", "mfma"), (2048, 200, 4096, 0.5, "mfma", "mfma")]


def ids(cases):
    return [f"{c[5]}-{c[0]}x{c[1]}x{c[2]}" for c in cases]


def make_plan(torch, env, Wd, path, slices=None, M=None, c0=0, c1=None):
    env(TCSC_PATH=path, TCSC_SLICES=slices)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan(W, c0, W.cols if c1 is None else c1)
    if M:
        plan.reserve(M)  # both calls then see the same workspace, so the same K split
    return W, plan


# ---- 1. the bits of the fp32 call on X.float(), 2. integers exact against numpy ------------------------------

@pytest.mark.parametrize("mode", ["plain", "slices3", "unaligned", "pitch"])
@pytest.mark.parametrize("case", GATHER, ids=ids(GATHER))
def test_gather_bits_of_the_fp32_call_and_exact_integers(gpu, oracle, env, case, mode):
    torch = gpu
    M, K, N, density, path, want_path = case
    c = int_case(oracle, M, K, N, density)
    W, plan = make_plan(torch, env, c["Wd"], path, slices=3 if mode == "slices3" else None, M=M)
    Xb = dev_bf16(torch, bf16_bits(c["X"]), offset=1 if mode == "unaligned" else 0)
    assert (Xb.data_ptr() % 16 != 0) == (mode == "unaligned")
    Xf, B = Xb.float(), dev_f32(torch, c["B"])
    assert plan.launch_info_bf16(M) == plan.launch_info(M)
    assert plan.launch_info_bf16(M)[0] == want_path
    if mode == "slices3" and K == 101:  # 3 chunks of K; K = 96 has 2, which a forced 3 cannot split
        assert plan.launch_info_bf16(M)[1] == 3
    ldy = N + 3 if mode == "pitch" else N
    fbits, fB = float_case(oracle, M, K, N)
    Xfb, FB = dev_bf16(torch, fbits, offset=1 if mode == "unaligned" else 0), dev_f32(torch, fB)
    for variant in pyoracle.VARIANTS:
        Yb = call(torch, plan, Xb, B, M, N, variant, True, ldy)
        Yf = call(torch, plan, Xf, B, M, N, variant, False, ldy)
        assert_same_bits(Yb, Yf, f"{mode}/{variant}")
        np.testing.assert_array_equal(Yb, exact(c, variant), err_msg=f"{mode}/{variant}")
        assert_same_bits(call(torch, plan, Xfb, FB, M, N, variant, True, ldy, a=0.2),
                         call(torch, plan, Xfb.float(), FB, M, N, variant, False, ldy, a=0.2),
                         f"{mode}/{variant}/float")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("case", SMALL + MFMA, ids=ids(SMALL + MFMA))
def test_small_and_mfma_bits_of_the_fp32_call_and_exact_integers(gpu, oracle, env, case):
    torch = gpu
    M, K, N, density, path, want_path = case
    c = int_case(oracle, M, K, N, density)
    W, plan = make_plan(torch, env, c["Wd"], path, M=M)
    Xb = dev_bf16(torch, bf16_bits(c["X"]))
    Xf, B = Xb.float(), dev_f32(torch, c["B"])
    assert plan.launch_info_bf16(M) == plan.launch_info(M)
    assert plan.launch_info_bf16(M)[0] == want_path
    if (M, K) == (40, 1100):
        assert plan.launch_info_bf16(M)[1] > 1  # narrow tiles, K split: k_reduce_fix
    fbits, fB = float_case(oracle, M, K, N)
    Xfb, FB = dev_bf16(torch, fbits), dev_f32(torch, fB)
    for variant in pyoracle.VARIANTS:
        Yb = call(torch, plan, Xb, B, M, N, variant, True)
        Yf = call(torch, plan, Xf, B, M, N, variant, False)
        assert_same_bits(Yb, Yf, variant)
        np.testing.assert_array_equal(Yb, exact(c, variant), err_msg=variant)
        assert_same_bits(call(torch, plan, Xfb, FB, M, N, variant, True, a=0.2),
                         call(torch, plan, Xfb.float(), FB, M, N, variant, False, a=0.2), f"{variant}/float")
    plan.destroy()
    W.free()


# ---- 3. float inputs within the library's bound of the exact fp64 sums ------------------------------------------

@pytest.mark.parametrize("case", [MFMA[0], GATHER[1]], ids=ids([MFMA[0], GATHER[1]]))
def test_float_within_bound(gpu, oracle, env, case):
    torch = gpu
    M, K, N, density, path, want_path = case
    Wd = oracle.ternary((K, N), density, 8100 + K)
    bits = bf16_bits(oracle.uniform((M, K), 8101 + K))
    Bh = oracle.uniform((N,), 8102 + K)
    Y64, S64 = oracle.f64_rows(widen(bits), oracle.tcsc_from_dense(Wd), Bh)
    W, plan = make_plan(torch, env, Wd, path, M=M)
    assert plan.launch_info_bf16(M)[0] == want_path
    Xb, B = dev_bf16(torch, bits), dev_f32(torch, Bh)
    for variant in pyoracle.VARIANTS:
        Y = call(torch, plan, Xb, B, M, N, variant, True, a=0.2)
        ok, ratio = pyoracle.check_close(Y, Y64, S64, 0.2 if variant in pyoracle.PRELU_VARIANTS else None)
        print(f"{want_path} {variant}: worst err/bound {ratio:.3g}")
        assert ok, f"{variant}: worst err/bound {ratio:.3g}"
    plan.destroy()
    W.free()


# ---- 4. rows the MFMA path cannot carry -----------------------------------------------------------------------

def test_mfma_special_rows_equal_the_gather_and_flags_are_rewritten(gpu, oracle, env):
    torch = gpu
    M, K, N, density = 200, 700, 300, 0.5
    c = int_case(oracle, M, K, N, density)
    clean = bf16_bits(c["X"])
    special = clean.copy()
    tiny = 17 << 7  # 2^-110: a normal bf16 below 2^-100
    assert widen(np.array([tiny], np.uint16))[0] == np.float32(2.0 ** -110)
    special[3, 17] = 0x7F80    # +inf
    special[10, 0] = 0xFF80    # -inf
    special[20, 100] = 0x7FC0  # NaN
    special[30, 5] = 0x0001    # a bf16 denormal
    special[31, 6] = tiny
    # and two rows of nothing but such values, where they are the whole sum (no bias in the first columns)
    special[150, :] = 0x0001
    special[160, :] = tiny
    Bh = c["B"].copy()
    Bh[:16] = 0.0
    out = {}
    for path in ("gather", "mfma"):
        W, plan = make_plan(torch, env, c["Wd"], path, slices=1, M=M)  # the gather unsplit: one accumulator per output
        assert plan.launch_info_bf16(M) == (path, 1)
        B = dev_f32(torch, Bh)
        Xb = dev_bf16(torch, special)
        runs = []
        for bits in (special, clean, special):  # one plan: the flags must follow X on every call
            Xb.copy_(dev_bf16(torch, bits))
            runs.append(call(torch, plan, Xb, B, M, N, "prelu_basic", True))
        out[path] = runs
        plan.destroy()
        W.free()
    g_special, g_clean, _ = out["gather"]
    assert np.isnan(g_special[[3, 10, 20]]).any() and np.isinf(g_special[[3, 10]]).any()
    assert (g_special[160, :16] != 0).any()  # the tiny values are the whole sum there
    assert np.isfinite(g_clean).all()
    for i, want in enumerate((g_special, g_clean, g_special)):
        assert_same_bits(out["mfma"][i], want, f"call {i}")


# ---- 5. plans of other kinds ------------------------------------------------------------------------------------

def test_transposed_plan(gpu, oracle, env):
    """sgemm_bf16 of bf16 G on the transposed plan: G.float() @ W^T, exact on integers."""
    torch = gpu
    env()
    M, K, N = 70, 96, 80
    Wd = oracle.ternary((K, N), 0.1, 8300)
    G = oracle.integers((M, N), 8301, rng=128)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    tplan = tcsc_amd.Plan.transposed(W)
    zero = torch.zeros(K, device=torch.device("cuda:0"))
    DX = call(torch, tplan, dev_bf16(torch, bf16_bits(G)), zero, M, K, "sparse_gemm", True)
    want = (G.astype(np.float64) @ Wd.astype(np.float64).T).astype(np.float32)
    np.testing.assert_array_equal(DX, want)
    tplan.destroy()
    W.free()


@pytest.mark.parametrize("path", ["gather", "mfma"])
def test_column_shard(gpu, oracle, env, path):
    torch = gpu
    M, K, N, c0, c1 = 200, 700, 300, 16, 208
    c = int_case(oracle, M, K, N, 0.5)
    W, plan = make_plan(torch, env, c["Wd"], path, M=M, c0=c0, c1=c1)
    assert plan.launch_info_bf16(M)[0] == path
    Y = call(torch, plan, dev_bf16(torch, bf16_bits(c["X"])), dev_f32(torch, c["B"][c0:c1]), M, c1 - c0,
             "prelu_basic", True, ldy=c1 - c0 + 5)
    np.testing.assert_array_equal(Y, c["act"][:, c0:c1])
    plan.destroy()
    W.free()


def test_reference_order_plan_takes_the_gather_with_the_fp32_bits(gpu, oracle, env):
    torch = gpu
    env()
    M, K, N = 70, 101, 80
    Wd = oracle.ternary((K, N), 0.5, 8400)
    bits = bf16_bits(oracle.uniform((M, K), 8401))
    tcsc_amd.set_order("reference")
    try:
        W = tcsc_amd.TcscMatrix.from_dense(Wd)
        plan = tcsc_amd.Plan(W)
        plan.reserve(M)
        assert plan.info()["order"] == 1
        assert plan.launch_info_bf16(M) == ("gather", 1)
        Xb, B = dev_bf16(torch, bits), dev_f32(torch, oracle.uniform((N,), 8402))
        for variant in pyoracle.VARIANTS:
            assert_same_bits(call(torch, plan, Xb, B, M, N, variant, True, a=0.2),
                             call(torch, plan, Xb.float(), B, M, N, variant, False, a=0.2), variant)
        plan.destroy()
        W.free()
    finally:
        tcsc_amd.set_order("fast")
        tcsc_amd.cache_clear()


# ---- 6. workspace and capture -----------------------------------------------------------------------------------

def test_reserve_covers_bf16_launches_and_a_captured_call_replays(gpu, oracle, env):
    torch = gpu
    env()
    dev = torch.device("cuda:0")
    K = N = 1024
    c = int_case(oracle, 256, K, N, 0.5)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    side = torch.cuda.Stream()
    plan = tcsc_amd.Plan(W, 0, N, 0, side.cuda_stream)
    plan.reserve(256)
    held = plan.info()["device_bytes"]
    Xb, B = dev_bf16(torch, bf16_bits(c["X"])), dev_f32(torch, c["B"])
    paths = set()
    for M in (1, 4, 5, 40, 64, 200, 256):
        paths.add(plan.launch_info_bf16(M)[0])
        Y = torch.empty((M, N), device=dev)
        with torch.cuda.stream(side):
            plan.sgemm_bf16(Xb, B, Y, M, N, "prelu_basic", A, side.cuda_stream)
        side.synchronize()
        assert plan.info()["device_bytes"] == held, f"M={M}: a bf16 call grew the plan"
        np.testing.assert_array_equal(Y.cpu().numpy(), c["act"][:M], err_msg=f"M={M}")
    assert {"small", "mfma"} <= paths
    # one captured call at M = 200, replayed on new X contents
    M = 200
    Xg = dev_bf16(torch, bf16_bits(c["X"][:M]))
    Yg = torch.empty((M, N), device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm_bf16(Xg, B, Yg, M, N, "prelu_basic", A, torch.cuda.current_stream().cuda_stream)
    for X2, want in ((c["X"][:M], c["act"][:M]), (c["X"][56:56 + M], c["act"][56:56 + M])):
        Xg.copy_(dev_bf16(torch, bf16_bits(X2)))
        Yg.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(Yg.cpu().numpy(), want)
    assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()


def test_bad_arguments_on_a_live_plan(gpu, oracle, env):
    torch = gpu
    env()
    c = int_case(oracle, 70, 96, 80, 0.1)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan(W)
    Xb, B = dev_bf16(torch, bf16_bits(c["X"])), dev_f32(torch, c["B"])
    Y = torch.empty((70, 80), device=Xb.device)
    L = tcsc_amd.lib()
    import ctypes as C

    def raw(M, ldy, variant, x=Xb):
        return L.tcsc_gpu_sgemm_bf16(plan.handle, C.c_void_p(x.data_ptr() if x is not None else 0),
                                     C.c_void_p(B.data_ptr()), C.c_void_p(Y.data_ptr()), M, ldy, variant, 0.2, None)

    assert raw(70, 80, 6) == 1 and raw(70, 80, -1) == 1   # bad variant
    assert raw(-1, 80, 0) == 1 and raw(70, 79, 0) == 1     # negative M, ldy < cols
    assert raw(70, 80, 0, x=None) == 1                     # NULL X
    assert raw(0, 80, 0) == 0                              # M = 0: nothing to do
    plan.destroy()
    W.free()


# ---- 7. the layer -----------------------------------------------------------------------------------------------

def test_layer_takes_bf16_and_keeps_fp32_as_it_was(gpu, oracle, env):
    torch = gpu
    env()
    from tcsc_amd.nn import TernaryLinear

    M, K, N = 24, 96, 80
    c = int_case(oracle, M, K, N, 0.1)
    G = oracle.integers((M, N), 8500, rng=64)
    layer = TernaryLinear(c["Wd"], bias=c["B"], a=A)
    info_before = layer.plan.launch_info(M)
    g = dev_f32(torch, G)

    x32 = dev_f32(torch, c["X"]).requires_grad_(True)
    y32 = layer(x32)
    y32.backward(g)

    xb = dev_bf16(torch, bf16_bits(c["X"])).detach().clone().requires_grad_(True)
    yb = layer(xb)
    assert yb.dtype == torch.float32 and yb.shape == (M, N)
    yb.backward(g)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(yb.detach().cpu().numpy(), y32.detach().cpu().numpy())
    np.testing.assert_array_equal(yb.detach().cpu().numpy(), c["act"])
    assert xb.grad.dtype == torch.bfloat16 and x32.grad.dtype == torch.float32
    assert torch.equal(xb.grad, x32.grad.to(torch.bfloat16))

    # fp32 x afterwards: the old path, the old bits
    assert layer.plan.launch_info(M) == info_before
    Yp = torch.empty((M, N), device=g.device)
    layer.plan.sgemm(x32.detach(), layer.bias.detach(), Yp, M, N, "prelu_basic", A)
    y32b = layer(x32.detach()).detach()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y32b.cpu().numpy().view(np.uint32), Yp.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(y32b.cpu().numpy().view(np.uint32), y32.detach().cpu().numpy().view(np.uint32))
    with pytest.raises(tcsc_amd.TcscError):
        layer(x32.detach().double())
