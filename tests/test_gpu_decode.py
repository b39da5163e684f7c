"""The int8 decode path: tcsc_gpu_sgemm_i8 calls of M <= 16 rows on the 2-bit image of W (k_decode8).

The yardsticks are numpy on the exact integer sums (held exactly by fp64 here: every |S| is asserted below 2^24)
through the float32 formula Y = act(fl(fl(float32(S)) * s) + b), and the library's existing paths under
TCSC_DECODE=0 -- never the decode call itself.  Plans are made under TCSC_PATH=mfma so that small and sparse W get
the images; every case checks that launch_info_i8 names `decode`.

Shapes are the smallest at which the kernel can go wrong: K around the 16-byte fragment, the 64-k MFMA step, the
256-k block and the 8 waves' K split (2048 k per round); N around the 16-column tile and, on a 256-CU chip, the
widths from which a workgroup owns 2 and 4 column tiles (513 and 1025 tiles, ragged last workgroups)."""
import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

A = 0.25  # exact on integers
ALL_VARIANTS = pyoracle.VARIANTS + ("sparse_gemm",)
PRELU = pyoracle.PRELU_VARIANTS
KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_DECODE")


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    import torch

    return torch


@pytest.fixture
def env(monkeypatch):
    """env(TCSC_PATH=..., TCSC_DECODE=...): the knobs for plans and calls made from now on."""

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


def assert_same_bits(got, want, what):
    assert not np.isnan(want).any() and not np.isnan(got).any(), what
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def int_sums(Xq, Wd):
    """S = q . W as int64.  fp64 holds these sums exactly (|S| < 2^24 is asserted), so BLAS computes them."""
    S = Xq.astype(np.float64) @ Wd.astype(np.float64)
    assert np.abs(S).max(initial=0) < 2 ** 24 and np.array_equal(S, np.rint(S))
    return S.astype(np.int64)


def formula(S, s, b, variant, a=A):
    """The contract in float32: act(fl(fl(float32(S)) * s) + b)."""
    v = S.astype(np.float32)
    if s is not None:
        v = v * np.asarray(s, np.float32)[:, None]
    v = v + np.asarray(b, np.float32)[None, :]
    assert v.dtype == np.float32
    return np.where(v < 0, np.float32(a) * v, v) if variant in PRELU else v


_cases = {}


def case(o, K, N, density=0.67, nnz=None):
    """W (of that density, or with exactly nnz nonzeros), a full-range 16-row int8 X (a row of all -128 and a run of
    127 among them), an integer and a float bias, power-of-two and float row scales, and the exact sums -- computed
    once per shape and left unchanged.  A test of M rows uses the first M."""
    key = (K, N, density, nnz)
    if key not in _cases:
        seed = 17000 + 3 * K + 5 * N + int(100 * density)
        rng = np.random.default_rng(seed)
        if nnz is None:
            Wd = o.ternary((K, N), density, seed)
        else:
            Wd = np.zeros(K * N, np.float32)
            Wd[rng.choice(K * N, nnz, replace=False)] = rng.choice(np.array([-1.0, 1.0], np.float32), nnz)
            Wd = Wd.reshape(K, N)
        Xq = rng.integers(-128, 128, (16, K), dtype=np.int64).astype(np.int8)
        Xq[2, :] = -128
        Xq[15, : K // 2 + 1] = 127
        Bi = o.integers((N,), seed + 2)
        Bf = o.uniform((N,), seed + 3)
        s2 = np.float32(2.0) ** rng.integers(-6, 4, 16).astype(np.float32)
        sf = (np.abs(o.uniform((16,), seed + 4)) * np.float32(0.05) + np.float32(1e-3)).astype(np.float32)
        _cases[key] = dict(Wd=Wd, Xq=Xq, Bi=Bi, Bf=Bf, s2=s2, sf=sf, S=int_sums(Xq, Wd))
    return _cases[key]


def make_plan(torch, env, Wd, path="mfma", c0=0, c1=None, w2=True, **knobs):
    env(TCSC_PATH=path, **knobs)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan(W, c0, W.cols if c1 is None else c1)
    plan.reserve(17)
    plan.enable_i8()
    if w2:
        assert plan.has_i8
        held = plan.info()["device_bytes"]
        assert plan.enable_w2() is True and plan.has_w2
        nc = plan.info()["cols"]
        assert plan.info()["device_bytes"] == held + tcsc_amd.w2_image_bytes(Wd.shape[0], nc)
        assert plan.enable_w2() is True and plan.info()["device_bytes"] == held + tcsc_amd.w2_image_bytes(Wd.shape[0], nc)
    return W, plan


def check_float(torch, plan, c, M, N, cols=slice(None), variant="prelu_basic", what=""):
    """Float scales and a float bias against the formula, bit for bit, on the decode path."""
    assert plan.launch_info_i8(M) == ("decode", 1), (what, M, plan.launch_info_i8(M))
    Y = call8(torch, plan, dev_i8(torch, c["Xq"][:M]), dev_f32(torch, c["sf"][:M]), dev_f32(torch, c["Bf"][cols]), M, N,
              variant, a=0.2)
    assert_same_bits(Y, formula(c["S"][:M, cols], c["sf"][:M], c["Bf"][cols], variant, a=0.2), f"{what} M={M}")
    return Y


# ---- 1. shape edges -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4112])
def test_k_edges(gpu, oracle, env, K):
    """K % 16 != 0 takes the guarded byte loads of X, K % 16 == 0 the 16-B ones (X 16-B aligned here); 1000 leaves
    four of the eight waves without a block, 4112 gives wave 0 three blocks and the others two."""
    torch = gpu
    N = 100
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"])
    for M in (1, 3, 16):
        check_float(torch, plan, c, M, N, what=f"K={K}")
    plan.destroy()
    W.free()


# on 256 CUs: 8200 columns are 513 tiles, where a workgroup owns 2 (M > 4) with a ragged last workgroup; 16400 are
# 1025, where it owns 4 (M > 8), 2 (M = 5 .. 8) or 1.  The narrowest plans take K = 64: a plan keeps its merged CSC
# copy, and with it the MFMA images, only while the copy's padding to 64-column groups stays within four times the
# nonzeros, which a few long columns do not (build_csc, csrc/tcsc_api.cpp).
@pytest.mark.parametrize("N,K,Ms", [(1, 64, (1, 3, 16)), (15, 64, (1, 3, 16)), (16, 64, (1, 3, 16)),
                                    (17, 64, (1, 3, 16)), (100, 300, (1, 3, 16)), (1030, 300, (1, 3, 16)),
                                    (8200, 260, (3, 8, 16)), (16400, 260, (3, 8, 16))],
                         ids=lambda v: str(v) if isinstance(v, int) else None)
def test_n_edges(gpu, oracle, env, N, K, Ms):
    torch = gpu
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"])
    for M in Ms:
        check_float(torch, plan, c, M, N, what=f"N={N}")
    plan.destroy()
    W.free()


def test_every_m_at_a_ragged_shape(gpu, oracle, env):
    torch = gpu
    K, N = 333, 77
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"])
    assert all(plan.workspace(M, "decode")[0] == 0 for M in (1, 16, 17))  # X is read in place
    for M in range(1, 17):
        check_float(torch, plan, c, M, N, what="ragged")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("density", [0.1, 0.67, 1.0])
def test_densities(gpu, oracle, env, density):
    torch = gpu
    K, N = 257, 100
    c = case(oracle, K, N, density)
    W, plan = make_plan(torch, env, c["Wd"])
    for M in (1, 3, 16):
        check_float(torch, plan, c, M, N, what=f"density {density}")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("w", [1, -1, 0])
def test_extremes(gpu, oracle, env, w):
    """W all +1, all -1 or all zero against q all -128 and all 127 at K = 4096: the largest sums the codes
    c = w + 1 and the row-sum correction see (|sum q c| = 2^20, |sum q| = 2^19)."""
    torch = gpu
    K, N = 4096, 48
    Wd = np.full((K, N), w, np.float32)
    W, plan = make_plan(torch, env, Wd)
    if w == 0:  # no nonzeros: the byte rule leaves M <= 4 to the small-M path
        assert plan.launch_info_i8(1)[0] != "decode"
        env(TCSC_PATH="mfma", TCSC_DECODE="1")
    Bi = oracle.integers((N,), 17901)
    for q in (-128, 127):
        for M in (1, 16):
            Xq = np.full((M, K), q, np.int8)
            S = int_sums(Xq, Wd)
            assert np.all(S == q * w * K)
            assert plan.launch_info_i8(M) == ("decode", 1)
            Y = call8(torch, plan, dev_i8(torch, Xq), None, dev_f32(torch, Bi), M, N, "prelu_basic")
            np.testing.assert_array_equal(Y, formula(S, None, Bi, "prelu_basic"), err_msg=f"w={w} q={q} M={M}")
    plan.destroy()
    W.free()


# ---- 2. the formula, bit for bit --------------------------------------------------------------------------------------

def test_bits_equal_the_formula(gpu, oracle, env):
    torch = gpu
    K, N = 333, 77
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"])
    for M in (3, 16):
        assert plan.launch_info_i8(M) == ("decode", 1)
        Xq = dev_i8(torch, c["Xq"][:M])
        Bi, Bf = dev_f32(torch, c["Bi"]), dev_f32(torch, c["Bf"])
        S2, Sf = dev_f32(torch, c["s2"][:M]), dev_f32(torch, c["sf"][:M])
        S = c["S"][:M]
        assert np.abs(S + c["Bi"].astype(np.int64)).max() < 2 ** 24  # exact in fp32
        for variant in ALL_VARIANTS:
            # integers: scale NULL and powers of two, PReLU with a = 0.25 -- exact
            np.testing.assert_array_equal(call8(torch, plan, Xq, None, Bi, M, N, variant),
                                          formula(S, None, c["Bi"], variant), err_msg=f"{variant}/s=NULL")
            np.testing.assert_array_equal(call8(torch, plan, Xq, S2, Bi, M, N, variant),
                                          formula(S, c["s2"][:M], c["Bi"], variant), err_msg=f"{variant}/s=2^e")
            # arbitrary fp32 scales and a float bias: the multiply and the add are rounded apart
            assert_same_bits(call8(torch, plan, Xq, Sf, Bf, M, N, variant, a=0.2),
                             formula(S, c["sf"][:M], c["Bf"], variant, a=0.2), f"{variant}/float")
        # ldy > N: the sentinel columns stay (call8 checks them)
        assert_same_bits(call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", N + 5, a=0.2),
                         formula(S, c["sf"][:M], c["Bf"], "prelu_basic", a=0.2), "pitch")
        # X one byte into its allocation: the byte loads
        Xu = dev_i8(torch, c["Xq"][:M], offset=1)
        assert Xu.data_ptr() % 16 == 1
        assert_same_bits(call8(torch, plan, Xu, Sf, Bf, M, N, "prelu_basic", a=0.2),
                         formula(S, c["sf"][:M], c["Bf"], "prelu_basic", a=0.2), "unaligned")
    plan.destroy()
    W.free()


def test_unaligned_x_with_k_a_multiple_of_16(gpu, oracle, env):
    """K = 256 would take the 16-B loads; one byte off they may not be used."""
    torch = gpu
    K, N = 256, 100
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"])
    for M in (1, 16):
        assert plan.launch_info_i8(M) == ("decode", 1)
        Xu = dev_i8(torch, c["Xq"][:M], offset=1)
        assert_same_bits(call8(torch, plan, Xu, dev_f32(torch, c["sf"][:M]), dev_f32(torch, c["Bf"]), M, N,
                               "prelu_basic", a=0.2),
                         formula(c["S"][:M], c["sf"][:M], c["Bf"], "prelu_basic", a=0.2), f"M={M}")
    plan.destroy()
    W.free()


# ---- 3. against the paths the library had -----------------------------------------------------------------------------

def test_bits_equal_k_gemm8s(gpu, oracle, env):
    torch = gpu
    K, N = 1000, 300
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"])
    for M in (5, 8, 16):
        Xq, Sf, Bf = dev_i8(torch, c["Xq"][:M]), dev_f32(torch, c["sf"][:M]), dev_f32(torch, c["Bf"])
        got = {}
        for knob, path in ((None, "decode"), ("0", "mfma")):
            env(TCSC_PATH="mfma", TCSC_DECODE=knob)
            assert plan.launch_info_i8(M)[0] == path, (M, knob, plan.launch_info_i8(M))
            for variant in ("prelu_basic", "sparse_gemm"):
                got[knob, variant] = call8(torch, plan, Xq, Sf, Bf, M, N, variant, a=0.2)
        for variant in ("prelu_basic", "sparse_gemm"):
            assert_same_bits(got[None, variant], got["0", variant], f"M={M}/{variant}")
            assert_same_bits(got["0", variant], formula(c["S"][:M], c["sf"][:M], c["Bf"], variant, a=0.2), "k_gemm8")
    plan.destroy()
    W.free()


def test_small_m_path_agrees_where_both_are_exact(gpu, oracle, env):
    """A default-built plan (no TCSC_PATH) of a dense-ish W routes M <= 4 to `decode` by the byte rule and to
    `small` under TCSC_DECODE=0.  k_small_m's contract is the fp32 call's bits on s * q; with s NULL and |S| < 2^24
    both paths are exact, so they agree bit for bit."""
    torch = gpu
    K, N = 256, 256
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"], path=None)
    nnz = plan.info()["nnz"]
    assert 16 * nnz > K * N and tcsc_amd.decode_pays(1, K, N, nnz)
    assert np.abs(c["S"] + c["Bi"].astype(np.int64)).max() < 2 ** 24
    for M in (1, 3, 4):
        Xq, Bi = dev_i8(torch, c["Xq"][:M]), dev_f32(torch, c["Bi"])
        env()
        assert plan.launch_info_i8(M) == ("decode", 1)
        Yd = call8(torch, plan, Xq, None, Bi, M, N, "prelu_basic")
        env(TCSC_DECODE="0")
        assert plan.launch_info_i8(M)[0] == "small"
        Ys = call8(torch, plan, Xq, None, Bi, M, N, "prelu_basic")
        assert_same_bits(Yd, Ys, f"M={M}")
        np.testing.assert_array_equal(Yd, formula(c["S"][:M], None, c["Bi"], "prelu_basic"))
    # a sparse W on a default-built plan stays on the small-M path at M <= 4 (16 nnz <= K N) unless TCSC_DECODE=1
    cs = case(oracle, K, N, nnz=3900)  # density 0.0595: above the MFMA image's 0.055, below the rule's 1/16
    Ws, sparse = make_plan(torch, env, cs["Wd"], path=None)
    assert sparse.info()["nnz"] == 3900 and 16 * 3900 <= K * N
    assert sparse.launch_info_i8(4)[0] == "small" and sparse.launch_info_i8(5)[0] == "decode"
    env(TCSC_DECODE="1")
    assert sparse.launch_info_i8(4) == ("decode", 1)
    check_float(torch, sparse, cs, 4, N, what="sparse, forced")
    for p, w in ((plan, W), (sparse, Ws)):
        p.destroy()
        w.free()


def test_m17_never_decodes_and_other_types_never_do(gpu, oracle, env):
    torch = gpu
    K, N = 333, 77
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"])
    rng = np.random.default_rng(17017)
    Xq = rng.integers(-128, 128, (17, K), dtype=np.int64).astype(np.int8)
    S = int_sums(Xq, c["Wd"])
    sf = np.linspace(0.01, 0.02, 17).astype(np.float32)
    for knob in (None, "1"):
        env(TCSC_PATH="mfma", TCSC_DECODE=knob)
        assert plan.launch_info_i8(16)[0] == "decode"
        assert plan.launch_info_i8(17)[0] == "mfma"
        for M in (1, 4, 16, 17):
            assert plan.launch_info(M)[0] != "decode" and plan.launch_info_bf16(M)[0] != "decode"
        Y = call8(torch, plan, dev_i8(torch, Xq), dev_f32(torch, sf), dev_f32(torch, c["Bf"]), 17, N, "prelu_basic",
                  a=0.2)
        assert_same_bits(Y, formula(S, sf, c["Bf"], "prelu_basic", a=0.2), f"M=17 knob={knob}")
    env(TCSC_PATH="mfma", TCSC_DECODE="0")
    assert all(plan.launch_info_i8(M)[0] == "mfma" for M in (1, 4, 5, 16))
    plan.destroy()
    W.free()


# ---- 4. plans that get no image -----------------------------------------------------------------------------------------

def test_a_duplicated_index_is_not_ternary(gpu, oracle, env):
    """A hand-built TCSC whose column 0 lists row 5 twice as +1 (|w| = 2): the int8 image holds it, the 2-bit image
    cannot.  enable_w2 returns OK and leaves the plan as it was; the int8 call gives what it gave before."""
    torch = gpu
    K, N, M = 200, 130, 16
    c = case(oracle, K, N)
    Wd = c["Wd"].copy()
    Wd[5, 0] = 0.0
    t = oracle.tcsc_from_dense(Wd)
    csp, rip = t.col_start_pos.astype(np.int64), t.row_index_pos
    n0 = int(csp[1])
    col0 = np.sort(np.concatenate([rip[:n0], np.full(2, 5, np.int32)])).astype(np.int32)
    rip2 = np.concatenate([col0, rip[n0:]]).astype(np.int32)
    csp2 = csp.copy()
    csp2[1:] += 2
    Weff = Wd.astype(np.float64)
    Weff[5, 0] = 2
    S = int_sums(c["Xq"], Weff)
    env(TCSC_PATH="mfma")
    dev = torch.device("cuda:0")
    arrs = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
            for a in (csp2.astype(np.int32), t.col_start_neg, rip2, t.row_index_neg)]
    plan = tcsc_amd.Plan.from_device(K, N, *arrs)
    plan.reserve(M)
    assert plan.enable_i8() is True
    Xq, Sf, Bf = dev_i8(torch, c["Xq"]), dev_f32(torch, c["sf"]), dev_f32(torch, c["Bf"])
    before = call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2)
    held, route = plan.info()["device_bytes"], [plan.launch_info_i8(m) for m in range(1, 18)]
    assert plan.enable_w2() is False and not plan.has_w2
    assert plan.info()["device_bytes"] == held and plan.has_i8
    assert [plan.launch_info_i8(m) for m in range(1, 18)] == route and all(r[0] != "decode" for r in route)
    env(TCSC_PATH="mfma", TCSC_DECODE="1")  # nothing to force
    assert plan.launch_info_i8(M)[0] == "mfma"
    after = call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2)
    assert_same_bits(after, before, "after enable_w2")
    assert_same_bits(after, formula(S, c["sf"], c["Bf"], "prelu_basic", a=0.2), "formula")
    plan.destroy()


def test_no_int8_image_no_2bit_image(gpu, oracle, env):
    torch = gpu
    K, N = 333, 77
    c = case(oracle, K, N)
    # a gather-only plan: enable_i8 leaves it as it was, and so does enable_w2
    W, plan = make_plan(torch, env, c["Wd"], path="gather", w2=False)
    assert not plan.has_i8
    held = plan.info()["device_bytes"]
    assert plan.enable_w2() is False and not plan.has_w2 and plan.info()["device_bytes"] == held
    env(TCSC_PATH="gather", TCSC_DECODE="1")
    assert plan.launch_info_i8(1)[0] != "decode" and plan.workspace(1, "decode")[0] == 0
    plan.destroy()
    W.free()
    # a plan with the bf16 image that never called enable_i8
    env(TCSC_PATH="mfma")
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan(W)
    assert plan.info()["mfma_min_M"] == 1 and not plan.has_i8
    assert plan.enable_w2() is False and not plan.has_w2
    plan.destroy()
    W.free()


# ---- 5. other plans -----------------------------------------------------------------------------------------------------

def test_column_shard(gpu, oracle, env):
    torch = gpu
    K, N = 333, 77
    c = case(oracle, K, N)
    c0, c1 = 5, 60  # col_begin > 0, 55 columns: three full tiles and a ragged one
    W, plan = make_plan(torch, env, c["Wd"], c0=c0, c1=c1)
    for M in (1, 3, 16):
        check_float(torch, plan, c, M, c1 - c0, cols=slice(c0, c1), what="shard")
    plan.destroy()
    W.free()


def test_transposed_plan(gpu, oracle, env):
    """sgemm_i8 of an int8 G on the transposed plan: G @ W^T, exact."""
    torch = gpu
    env(TCSC_PATH="mfma")
    M, K, N = 16, 96, 200
    Wd = oracle.ternary((K, N), 0.67, 17300)
    G = np.random.default_rng(17301).integers(-128, 128, (M, N), dtype=np.int64).astype(np.int8)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    tplan = tcsc_amd.Plan.transposed(W)
    tplan.reserve(M)
    assert tplan.enable_i8() and tplan.enable_w2()
    zero = torch.zeros(K, device=torch.device("cuda:0"))
    for m in (1, 3, 16):
        assert tplan.launch_info_i8(m) == ("decode", 1)
        DX = call8(torch, tplan, dev_i8(torch, G[:m]), None, zero, m, K, "sparse_gemm")
        np.testing.assert_array_equal(DX, int_sums(G[:m], Wd.T).astype(np.float32))
    tplan.destroy()
    W.free()


# ---- 6. capture -------------------------------------------------------------------------------------------------------

def test_a_captured_decode_call_replays_on_new_inputs(gpu, oracle, env):
    """One decode call at M = 1 captured on one stream, replayed with new X and scales: the call allocates nothing
    and keeps no state between launches."""
    torch = gpu
    K, N, M = 1000, 300, 1
    c = case(oracle, K, N)
    W, plan = make_plan(torch, env, c["Wd"])
    assert plan.launch_info_i8(M) == ("decode", 1)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()
    held = plan.info()["device_bytes"]
    Qg = torch.zeros((M, K), dtype=torch.int8, device=dev)
    Sg = torch.zeros(M, device=dev)
    Yg = torch.empty((M, N), device=dev)
    Bf = dev_f32(torch, c["Bf"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm_i8(Qg, Sg, Bf, Yg, M, N, "prelu_basic", 0.2, torch.cuda.current_stream().cuda_stream)
    for row in (0, 7):
        Qg.copy_(dev_i8(torch, c["Xq"][row:row + 1]))
        Sg.copy_(dev_f32(torch, c["sf"][row:row + 1]))
        Yg.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(Yg.cpu().numpy(),
                         formula(c["S"][row:row + 1], c["sf"][row:row + 1], c["Bf"], "prelu_basic", a=0.2),
                         f"replay with row {row}")
    assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()


# ---- 7. the layer -------------------------------------------------------------------------------------------------------

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


def test_layer_reserve_decode(gpu, oracle, env):
    torch = gpu
    env()
    from tcsc_amd.nn import TernaryLinear

    K, N = 300, 130
    c = case(oracle, K, N)
    X = oracle.uniform((4, K), 17501)
    plain = TernaryLinear(c["Wd"], bias=c["Bf"], a=0.2)
    plain.reserve(4, int8=True)
    assert plain.plan.has_i8 and not plain.plan.has_w2
    assert all(plain.plan.launch_info_i8(M)[0] != "decode" for M in (1, 4))
    layer = TernaryLinear(c["Wd"], bias=c["Bf"], a=0.2)
    with pytest.raises(tcsc_amd.TcscError):
        layer.reserve(4, decode=True)  # the 2-bit image is made from the int8 one
    layer.reserve(4, int8=True, decode=True)
    assert layer.plan.has_w2
    for M in (1, 4):
        assert layer.plan.launch_info_i8(M) == ("decode", 1)
        x = dev_f32(torch, X[:M])
        with torch.no_grad():
            y = layer.forward_int8(x)
            y0 = plain.forward_int8(x)
        torch.cuda.synchronize()
        q, s = np_quantize(X[:M])
        want = formula(int_sums(q, c["Wd"]), s, c["Bf"], "prelu_basic", a=0.2)
        assert_same_bits(y.cpu().numpy(), want, f"forward_int8 M={M}")
        assert y0.shape == y.shape
