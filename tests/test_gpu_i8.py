"""tcsc_gpu_sgemm_i8: int8 activations with a per-row scale on every path, and
tcsc_gpu_quantize_rows_i8.

The yardsticks are numpy on the exact integer sums (held exactly by fp64 here:
every |S| is asserted below 2^24), the fp32 call on Xs = s * q, and a numpy
restatement of the quantizer -- never the int8 call itself.  The MFMA path's
contract is Y = act(fl(fl(float32(S)) * s) + b) in float32, bit for bit, for
every variant and K split; the gather's and the small-M path's are the bits of
Plan.sgemm on Xs on the same plan, path and K split.  Every test forces its
path with $TCSC_PATH and checks launch_info_i8 names it.
"""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

A = 0.25  # exact on integers
ALL_VARIANTS = pyoracle.VARIANTS + ("sparse_gemm",)
PRELU = pyoracle.PRELU_VARIANTS
KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M")


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    import torch

    return torch


@pytest.fixture
def env(monkeypatch):
    """env(TCSC_PATH=..., TCSC_SLICES=..., TCSC_MFMA_WGS=...): the knobs for plans and calls made from now on."""

    def set_env(**kw):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            if v is not None:
                monkeypatch.setenv(k, str(v))
        tcsc_amd.cache_clear()

    yield set_env
    tcsc_amd.cache_clear()


def dev_i8(torch, q, offset=0):
    """A contiguous torch.int8 device tensor with these values, `offset` bytes into its allocation."""
    dev = torch.device("cuda:0")
    buf = torch.zeros(q.size + 32, dtype=torch.int8, device=dev)
    v = buf[offset:offset + q.size].view(*q.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(q, np.int8)).to(dev))
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + offset
    return v


def dev_f32(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.device("cuda:0"))


def call8(torch, plan, Xq, S, B, M, nc, variant, ldy=None, a=A):
    """One int8 launch into a sentinel-filled Y; the plan's columns of it, the sentinel columns checked."""
    ldy = ldy or nc
    Y = torch.full((M, ldy), 7.0, device=Xq.device)
    plan.sgemm_i8(Xq, S, B, Y, M, ldy, variant, a)
    torch.cuda.synchronize()
    Y = Y.cpu().numpy()
    assert np.all(Y[:, nc:] == 7.0), "columns beyond the plan's were written"
    return Y[:, :nc]


def call32(torch, plan, X, B, M, nc, variant, ldy=None, a=A):
    ldy = ldy or nc
    Y = torch.full((M, ldy), 7.0, device=X.device)
    plan.sgemm(X, B, Y, M, ldy, variant, a)
    torch.cuda.synchronize()
    return Y.cpu().numpy()[:, :nc]


def assert_same_bits(got, want, what):
    assert not np.isnan(want).any() and not np.isnan(got).any(), what
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def int_sums(Xq, Wd):
    """S = q . W as int64.  fp64 holds these sums exactly (|S| < 2^24 is asserted), so BLAS computes them."""
    S = Xq.astype(np.float64) @ Wd.astype(np.float64)
    assert np.abs(S).max() < 2 ** 24 and np.array_equal(S, np.rint(S))
    return S.astype(np.int64)


def formula(S, s, b, variant, a=A):
    """The MFMA contract in float32: act(fl(fl(float32(S)) * s) + b)."""
    v = S.astype(np.float32)
    if s is not None:
        v = v * np.asarray(s, np.float32)[:, None]
    v = v + np.asarray(b, np.float32)[None, :]
    assert v.dtype == np.float32
    return np.where(v < 0, np.float32(a) * v, v) if variant in PRELU else v


_cases = {}


def case(o, M, K, N, density=0.5):
    """W, a full-range int8 X (rows of all -128 among them), an integer and a float bias, power-of-two and float
    row scales, and the exact sums -- computed once per shape."""
    key = (M, K, N, density)
    if key not in _cases:
        seed = 9000 + M + 3 * K + 5 * N
        rng = np.random.default_rng(seed)
        Wd = o.ternary((K, N), density, seed)
        Xq = rng.integers(-128, 128, (M, K), dtype=np.int64).astype(np.int8)
        Xq[0, :] = -128
        Xq[M // 2, :] = -128
        Xq[M - 1, : K // 2 + 1] = 127
        Bi = o.integers((N,), seed + 2)
        Bf = o.uniform((N,), seed + 3)
        s2 = np.float32(2.0) ** rng.integers(-6, 4, M).astype(np.float32)
        sf = (np.abs(o.uniform((M,), seed + 4)) * np.float32(0.05) + np.float32(1e-3)).astype(np.float32)
        _cases[key] = dict(Wd=Wd, Xq=Xq, Bi=Bi, Bf=Bf, s2=s2, sf=sf, S=int_sums(Xq, Wd))
    return _cases[key]


def make_plan(torch, env, Wd, path, M=None, c0=0, c1=None, i8=True, **knobs):
    env(TCSC_PATH=path, **knobs)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan(W, c0, W.cols if c1 is None else c1)
    if M:
        plan.reserve(M)
    if i8:
        plan.enable_i8()
    return W, plan


# ---- 1. MFMA, exact integers --------------------------------------------------------------------------------------

# (M, K, N): one 128-k block (the tail reload), two blocks (127 bytes of padding), three (an odd count), ragged
# everywhere, narrow tiles, a 5-row call, big tiles
MFMA_SHAPES = [(200, 128, 300), (200, 129, 300), (200, 300, 300), (130, 701, 257), (40, 1100, 300), (5, 385, 130),
               (2048, 200, 4096)]


@pytest.mark.parametrize("shape", MFMA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mfma_exact_integers(gpu, oracle, env, shape):
    torch = gpu
    M, K, N = shape
    c = case(oracle, M, K, N)
    W, plan = make_plan(torch, env, c["Wd"], "mfma", M=M)
    assert plan.has_i8 and plan.enable_i8() is True  # idempotent
    Xq, B = dev_i8(torch, c["Xq"]), dev_f32(torch, c["Bi"])
    S2 = dev_f32(torch, c["s2"])
    forms = [("default", None)]
    if shape == (40, 1100, 300):
        assert plan.launch_info_i8(M) == ("mfma", plan.launch_info_i8(M)[1]) and plan.launch_info_i8(M)[1] > 1
        forms.append(("unsplit", "0"))
    for form, wgs in forms:
        env(TCSC_PATH="mfma", TCSC_MFMA_WGS=wgs)
        path, slices = plan.launch_info_i8(M)
        assert path == "mfma" and (form != "unsplit" or slices == 1)
        variants = ALL_VARIANTS if shape in ((200, 300, 300), (40, 1100, 300)) else ("prelu_basic", "basic")
        for variant in variants:
            want = formula(c["S"], None, c["Bi"], variant)
            assert np.abs(c["S"] + c["Bi"].astype(np.int64)).max() < 2 ** 24  # exact in fp32
            np.testing.assert_array_equal(call8(torch, plan, Xq, None, B, M, N, variant), want,
                                          err_msg=f"{form}/{variant}/s=NULL")
            np.testing.assert_array_equal(call8(torch, plan, Xq, S2, B, M, N, variant),
                                          formula(c["S"], c["s2"], c["Bi"], variant),
                                          err_msg=f"{form}/{variant}/s=2^e")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("mode", ["unaligned", "pitch", "shard"])
def test_mfma_unaligned_x_pitched_y_and_column_shard(gpu, oracle, env, mode):
    torch = gpu
    M, K, N = 200, 300, 300
    c = case(oracle, M, K, N)
    c0, c1 = (16, 208) if mode == "shard" else (0, N)
    W, plan = make_plan(torch, env, c["Wd"], "mfma", M=M, c0=c0, c1=c1)
    assert plan.has_i8 and plan.launch_info_i8(M)[0] == "mfma"
    Xq = dev_i8(torch, c["Xq"], offset=1 if mode == "unaligned" else 0)
    assert (Xq.data_ptr() % 16 != 0) == (mode == "unaligned")
    nc = c1 - c0
    ldy = nc if mode == "unaligned" else nc + 5
    Y = call8(torch, plan, Xq, dev_f32(torch, c["s2"]), dev_f32(torch, c["Bi"][c0:c1]), M, nc, "prelu_basic", ldy)
    np.testing.assert_array_equal(Y, formula(c["S"][:, c0:c1], c["s2"], c["Bi"][c0:c1], "prelu_basic"))
    plan.destroy()
    W.free()


# ---- 2. MFMA, general scales ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(200, 300, 300), (130, 701, 257), (40, 1100, 300), (2048, 200, 4096)],
                         ids=lambda s: "x".join(map(str, s)))
def test_mfma_float_scales_and_bias(gpu, oracle, env, shape):
    torch = gpu
    M, K, N = shape
    c = case(oracle, M, K, N)
    W, plan = make_plan(torch, env, c["Wd"], "mfma", M=M)
    assert plan.has_i8
    Xq, B, Sf = dev_i8(torch, c["Xq"]), dev_f32(torch, c["Bf"]), dev_f32(torch, c["sf"])
    got = {}
    for wgs in (None, "0"):
        env(TCSC_PATH="mfma", TCSC_MFMA_WGS=wgs)
        path, slices = plan.launch_info_i8(M)
        assert path == "mfma" and (wgs is None or slices == 1)
        for variant in ("prelu_basic", "sparse_gemm"):
            got[wgs, variant] = call8(torch, plan, Xq, Sf, B, M, N, variant, a=0.2)
            assert_same_bits(got[wgs, variant], formula(c["S"], c["sf"], c["Bf"], variant, a=0.2),
                             f"wgs={wgs}/{variant}")
    for variant in ("prelu_basic", "sparse_gemm"):
        assert_same_bits(got[None, variant], got["0", variant], f"split vs unsplit/{variant}")
    plan.destroy()
    W.free()


# ---- 3. split-K invariance ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", [(0, 600, 600), (3, 570, 571), (100, 229, 140)], ids=lambda b: f"{b[0]}-{b[1]}")
def test_split_k_invariance(gpu, oracle, env, block):
    torch = gpu
    M, K, N = 96, 3000, 600
    c0, c1, ldy = block
    c = case(oracle, M, K, N)
    W, plan = make_plan(torch, env, c["Wd"], "mfma", M=M, c0=c0, c1=c1)
    assert plan.has_i8
    nc = c1 - c0
    Xq, B, Sf = dev_i8(torch, c["Xq"]), dev_f32(torch, c["Bf"][c0:c1]), dev_f32(torch, c["sf"])
    want = formula(c["S"][:, c0:c1], c["sf"], c["Bf"][c0:c1], "prelu_basic", a=0.2)
    seen = set()
    for wgs in (None, "0"):
        env(TCSC_PATH="mfma", TCSC_MFMA_WGS=wgs)
        path, slices = plan.launch_info_i8(M)
        assert path == "mfma"
        seen.add(slices)
        assert_same_bits(call8(torch, plan, Xq, Sf, B, M, nc, "prelu_basic", ldy, a=0.2), want, f"wgs={wgs}")
    assert 1 in seen and max(seen) > 1, seen  # K split by default, unsplit with TCSC_MFMA_WGS=0
    plan.destroy()
    W.free()


# ---- 4. gather and small M: the bits of the fp32 call on Xs = s * q ----------------------------------------------------

# K = 144: a multiple of 16 past one 128-k tile -- the vector transpose's second k tile is mostly past K (its load
# and store guards), with a ragged second row tile.  K = 4112: a multiple of 16 past 4096 -- the small-M vector
# staging takes a second pass, on clamped addresses (small_m_fits(4, 4112): 131,712 bytes).
GATHER = [(70, 96, 80, 0.1, "gather", "gather"), (70, 101, 80, 0.1, "gather", "gather"),
          (70, 112, 80, 0.1, "gather", "gather"), (70, 144, 80, 0.1, "gather", "gather")]
SMALL = [(M, K, 130, 0.1, None, "small") for M in (1, 3, 4) for K in (96, 101, 112)] + \
        [(M, 4112, 130, 0.1, None, "small") for M in (1, 4)]


def ids(cases):
    return [f"{c[5]}-{c[0]}x{c[1]}x{c[2]}" for c in cases]


@pytest.mark.parametrize("slices", [None, 3], ids=["plain", "slices3"])
@pytest.mark.parametrize("cs", GATHER + SMALL, ids=ids(GATHER + SMALL))
def test_gather_and_small_bits_of_the_fp32_call(gpu, oracle, env, cs, slices):
    torch = gpu
    M, K, N, density, path, want_path = cs
    c = case(oracle, M, K, N, density)
    W, plan = make_plan(torch, env, c["Wd"], path, M=M, TCSC_SLICES=slices)
    # TCSC_PATH=gather plans hold no MFMA image and enable_i8 leaves them as they were; the small-M plans hold
    # both images and still serve M <= 4 from the small-M path
    assert plan.has_i8 == (path is None)
    assert plan.launch_info_i8(M) == plan.launch_info(M) and plan.launch_info_i8(M)[0] == want_path
    if want_path == "gather" and slices == 3 and K > 96:  # 3 chunks of K; K = 96 has 2
        assert plan.launch_info_i8(M)[1] == 3
    Xq = dev_i8(torch, c["Xq"])
    Xs = (c["sf"][:, None] * c["Xq"].astype(np.float32)).astype(np.float32)
    assert Xs.dtype == np.float32
    Bi, Bf, Sf = dev_f32(torch, c["Bi"]), dev_f32(torch, c["Bf"]), dev_f32(torch, c["sf"])
    X1, Xsd = dev_f32(torch, c["Xq"].astype(np.float32)), dev_f32(torch, Xs)
    for variant in ALL_VARIANTS:
        # integers, s = NULL: exact, and the fp32 call's bits
        Y = call8(torch, plan, Xq, None, Bi, M, N, variant)
        np.testing.assert_array_equal(Y, formula(c["S"], None, c["Bi"], variant), err_msg=variant)
        assert_same_bits(Y, call32(torch, plan, X1, Bi, M, N, variant), f"{variant}/int")
        # float scales and bias: the fp32 call on Xs, same plan, path and K split
        assert_same_bits(call8(torch, plan, Xq, Sf, Bf, M, N, variant, a=0.2),
                         call32(torch, plan, Xsd, Bf, M, N, variant, a=0.2), f"{variant}/float")
    # an X one byte off 16-B alignment takes the scalar staging: the same bits
    Xu = dev_i8(torch, c["Xq"], offset=1)
    assert_same_bits(call8(torch, plan, Xu, Sf, Bf, M, N, "prelu_basic", N + 3, a=0.2),
                     call32(torch, plan, Xsd, Bf, M, N, "prelu_basic", a=0.2), "unaligned")
    plan.destroy()
    W.free()


# ---- 5. plans without the image -------------------------------------------------------------------------------------

def test_sparse_and_reference_order_plans_have_no_image_and_run_the_gather(gpu, oracle, env):
    torch = gpu
    M, K, N = 70, 101, 80
    for what in ("sparse", "reference"):
        c = case(oracle, M, K, N, 0.05 if what == "sparse" else 0.5)
        if what == "reference":
            tcsc_amd.set_order("reference")
        try:
            W, plan = make_plan(torch, env, c["Wd"], "gather" if what == "sparse" else None, M=M)
            assert plan.enable_i8() is False and not plan.has_i8
            assert plan.launch_info_i8(M)[0] == "gather"
            Xq, B, Sf = dev_i8(torch, c["Xq"]), dev_f32(torch, c["Bf"]), dev_f32(torch, c["sf"])
            Xs = dev_f32(torch, (c["sf"][:, None] * c["Xq"].astype(np.float32)).astype(np.float32))
            for variant in ALL_VARIANTS:
                assert_same_bits(call8(torch, plan, Xq, Sf, B, M, N, variant, a=0.2),
                                 call32(torch, plan, Xs, B, M, N, variant, a=0.2), f"{what}/{variant}")
            np.testing.assert_array_equal(call8(torch, plan, Xq, None, dev_f32(torch, c["Bi"]), M, N, "prelu_basic"),
                                          formula(c["S"], None, c["Bi"], "prelu_basic"))
            plan.destroy()
            W.free()
        finally:
            tcsc_amd.set_order("fast")
            tcsc_amd.cache_clear()


@pytest.mark.parametrize("repeats", [127, 128])
def test_a_repeated_row_decides_the_image(gpu, oracle, env, repeats):
    """A hand-built TCSC whose column 0 lists row 5 `repeats` times as +1: |w| = 127 fits int8 and the image is
    built (exact); 128 does not, enable_i8 leaves the plan as it was and the call runs the gather, right."""
    torch = gpu
    M, K, N = 70, 200, 130
    c = case(oracle, M, K, N)
    Wd = c["Wd"].copy()
    Wd[5, 0] = 0.0
    t = oracle.tcsc_from_dense(Wd)
    csp, rip = t.col_start_pos.astype(np.int64), t.row_index_pos
    n0 = int(csp[1])  # column 0's +1 rows, ascending; row 5 goes in `repeats` times, in order
    col0 = np.sort(np.concatenate([rip[:n0], np.full(repeats, 5, np.int32)])).astype(np.int32)
    rip2 = np.concatenate([col0, rip[n0:]]).astype(np.int32)
    csp2 = csp.copy()
    csp2[1:] += repeats
    Weff = Wd.astype(np.float64)
    Weff[5, 0] = repeats
    S = int_sums(c["Xq"], Weff)
    env(TCSC_PATH="mfma")
    dev = torch.device("cuda:0")
    arrs = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
            for a in (csp2.astype(np.int32), t.col_start_neg, rip2, t.row_index_neg)]
    plan = tcsc_amd.Plan.from_device(K, N, *arrs)
    plan.reserve(M)
    assert plan.info()["mfma_min_M"] > 0  # the bf16 image holds 128 exactly
    held = plan.info()["device_bytes"]
    assert plan.enable_i8() == (repeats == 127) and plan.has_i8 == (repeats == 127)
    if repeats == 128:
        assert plan.info()["device_bytes"] == held
        assert plan.launch_info_i8(M)[0] == "gather" and plan.launch_info(M)[0] == "mfma"
    else:
        assert plan.info()["device_bytes"] == held + N * 256  # K = 200 rounds up to 256 bytes a column
        assert plan.launch_info_i8(M)[0] == "mfma"
    Y = call8(torch, plan, dev_i8(torch, c["Xq"]), dev_f32(torch, c["s2"]), dev_f32(torch, c["Bi"]), M, N,
              "prelu_basic")
    np.testing.assert_array_equal(Y, formula(S, c["s2"], c["Bi"], "prelu_basic"))
    plan.destroy()


# ---- 6. reserve and capture ------------------------------------------------------------------------------------------

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


def test_reserve_covers_i8_launches_and_a_captured_pipeline_replays(gpu, oracle, env):
    torch = gpu
    env()
    dev = torch.device("cuda:0")
    K = N = 1024
    c = case(oracle, 256, K, N)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    side = torch.cuda.Stream()
    plan = tcsc_amd.Plan(W, 0, N, 0, side.cuda_stream)
    plan.reserve(256)
    assert plan.enable_i8(side.cuda_stream)
    held = plan.info()["device_bytes"]
    Xq, B, S2 = dev_i8(torch, c["Xq"]), dev_f32(torch, c["Bi"]), dev_f32(torch, c["s2"])
    want = formula(c["S"], c["s2"], c["Bi"], "prelu_basic")
    paths = set()
    for M in (1, 4, 5, 17, 64, 128, 256):
        paths.add(plan.launch_info_i8(M)[0])
        Y = torch.empty((M, N), device=dev)
        with torch.cuda.stream(side):
            plan.sgemm_i8(Xq, S2, B, Y, M, N, "prelu_basic", A, side.cuda_stream)
        side.synchronize()
        assert plan.info()["device_bytes"] == held, f"M={M}: an int8 call grew the plan"
        np.testing.assert_array_equal(Y.cpu().numpy(), want[:M], err_msg=f"M={M}")
    assert {"small", "mfma"} <= paths
    # quantize + sgemm captured once at M = 200, replayed on new X written into the same buffer
    M = 200
    Xg = torch.empty((M, K), device=dev)
    Qg = torch.empty((M, K), dtype=torch.int8, device=dev)
    Sg = torch.empty(M, device=dev)
    Yg = torch.empty((M, N), device=dev)
    Bf = dev_f32(torch, c["Bf"])
    X1, X2 = oracle.uniform((M, K), 9901), oracle.uniform((M, K), 9902)
    Xg.copy_(dev_f32(torch, X1))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        st = torch.cuda.current_stream().cuda_stream
        tcsc_amd.quantize_rows_i8(Xg, Qg, Sg, M, K, st)
        plan.sgemm_i8(Qg, Sg, Bf, Yg, M, N, "prelu_basic", 0.2, st)
    for X in (X1, X2):
        Xg.copy_(dev_f32(torch, X))
        Yg.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        q, s = np_quantize(X)
        assert_same_bits(Yg.cpu().numpy(), formula(int_sums(q, c["Wd"]), s, c["Bf"], "prelu_basic", a=0.2), "replay")
    assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()


# ---- 7. the quantizer -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (3, 101), (70, 4096), (5, 16385)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantizer_equals_the_numpy_restatement(gpu, oracle, shape):
    torch = gpu
    M, K = shape
    X = oracle.uniform((M, K), 9700 + K)
    if M > 1:
        X[M - 1, :] = 0.0                  # a row of zeros: q = 0, scale = 0
        X[0, :] = np.abs(X[0, :]) * np.float32(0.5)
        X[0, K - 1] = -3.0                 # the row's amax sits in its last element
    if M > 2:
        # amax = 127: inv = 1, so n + 0.5 stays n + 0.5 and rint must round half to even
        X[1, :] = (np.arange(K) % 250 - 125).astype(np.float32) + np.float32(0.5)
        X[1, 0] = 127.0
    q, s = np_quantize(X)
    if M > 2:
        assert np.array_equal(q[1, 1:5], [-124, -122, -122, -120])  # -123.5, -122.5, -121.5, -120.5
    for offset in (0, 1):  # 16-B aligned buffers, and an Xq one byte off
        dev = torch.device("cuda:0")
        Xd = dev_f32(torch, X)
        buf = torch.full((M * K + 32,), 99, dtype=torch.int8, device=dev)
        Qd = buf[offset:offset + M * K].view(M, K)
        Sd = torch.full((M,), 7.0, device=dev)
        tcsc_amd.quantize_rows_i8(Xd, Qd, Sd, M, K)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(Qd.cpu().numpy(), q, err_msg=f"offset {offset}")
        np.testing.assert_array_equal(Sd.cpu().numpy().view(np.uint32), s.view(np.uint32), err_msg=f"offset {offset}")
        rest = buf.cpu().numpy()
        assert np.all(rest[:offset] == 99) and np.all(rest[offset + M * K:] == 99), "wrote outside Xq"
    assert M == 1 or (np.all(q[M - 1] == 0) and s[M - 1] == 0)


# ---- 8. transposed plan -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,density", [("gather", 0.1), ("mfma", 0.5)])
def test_transposed_plan(gpu, oracle, env, path, density):
    """sgemm_i8 of an int8 G on the transposed plan: G @ W^T, exact."""
    torch = gpu
    env(TCSC_PATH=path)
    M, K, N = 70, 96, 200
    Wd = oracle.ternary((K, N), density, 9300)
    G = np.random.default_rng(9301).integers(-128, 128, (M, N), dtype=np.int64).astype(np.int8)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    tplan = tcsc_amd.Plan.transposed(W)
    tplan.reserve(M)
    assert tplan.enable_i8() == (path == "mfma")
    assert tplan.launch_info_i8(M)[0] == path
    zero = torch.zeros(K, device=torch.device("cuda:0"))
    DX = call8(torch, tplan, dev_i8(torch, G), None, zero, M, K, "sparse_gemm")
    np.testing.assert_array_equal(DX, int_sums(G, Wd.T).astype(np.float32))
    tplan.destroy()
    W.free()


# ---- 9. bad arguments on a live plan ----------------------------------------------------------------------------------

def test_bad_arguments_on_a_live_plan(gpu, oracle, env):
    torch = gpu
    env(TCSC_PATH="gather")
    M, K, N = 70, 96, 80
    c = case(oracle, M, K, N, 0.1)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan(W)
    assert plan.launch_info_i8(M)[0] == "gather"
    Xq, B = dev_i8(torch, c["Xq"]), dev_f32(torch, c["Bi"])
    Y = torch.full((M, N), 7.0, device=Xq.device)
    L = tcsc_amd.lib()

    def raw(M_, ldy, variant, x=Xq, b=B, y=Y):
        p = [C.c_void_p(t.data_ptr() if t is not None else 0) for t in (x, b, y)]
        return L.tcsc_gpu_sgemm_i8(plan.handle, p[0], None, p[1], p[2], M_, ldy, variant, 0.2, None)

    assert raw(M, N, 6) == 1 and raw(M, N, -1) == 1                # bad variant
    assert raw(-1, N, 0) == 1 and raw(M, N - 1, 0) == 1            # negative M, ldy < cols
    assert raw(M, N, 0, x=None) == 1 and raw(M, N, 0, b=None) == 1 and raw(M, N, 0, y=None) == 1  # NULL X / B / Y
    assert "tcsc_gpu_sgemm_i8" in tcsc_amd.last_error()
    torch.cuda.synchronize()
    assert torch.all(Y == 7.0), "a rejected call wrote Y"
    assert raw(0, N, 0) == 0                                       # M = 0: nothing to do
    plan.destroy()
    W.free()


# ---- 10. the layer ----------------------------------------------------------------------------------------------------

def test_layer_forward_int8(gpu, oracle, env):
    torch = gpu
    env()
    from tcsc_amd.nn import TernaryLinear

    M, K, N = 70, 300, 130
    c = case(oracle, M, K, N)
    X = oracle.uniform((M, K), 9501)
    layer = TernaryLinear(c["Wd"], bias=c["Bf"], a=0.2)
    x = dev_f32(torch, X)
    before = layer(x).detach().cpu().numpy()
    info_before = layer.plan.launch_info(M)
    layer.reserve(M, int8=True)
    assert layer.plan.has_i8 and layer.plan.launch_info_i8(M)[0] == "mfma"
    with torch.no_grad():
        y = layer.forward_int8(x)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.shape == (M, N)
    q, s = np_quantize(X)
    assert_same_bits(y.cpu().numpy(), formula(int_sums(q, c["Wd"]), s, c["Bf"], "prelu_basic", a=0.2), "forward_int8")
    # leading dimensions are flattened and restored
    with torch.no_grad():
        y3 = layer.forward_int8(x.reshape(7, 10, K))
    assert y3.shape == (7, 10, N) and torch.equal(y3.reshape(M, N), y)
    # inference only
    with pytest.raises(tcsc_amd.TcscError):
        layer.forward_int8(x.clone().requires_grad_(True))
    with pytest.raises(tcsc_amd.TcscError):
        layer.forward_int8(x.double())
    # forward is what it was before the image existed
    assert layer.plan.launch_info(M) == info_before
    after = layer(x).detach().cpu().numpy()
    np.testing.assert_array_equal(after.view(np.uint32), before.view(np.uint32))
