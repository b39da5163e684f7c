"""Packed plans: the 2-bit image straight from TCSC (k_w2_from_tcsc) and tcsc_gpu_sgemm_i8 at every M
from that image alone (k_decode8 up to 16 rows, k_pack8 + k_gemm8w2 above).

Yardsticks, never the packed call itself:
  * the image: a numpy restatement of the layout include/tcsc_gpu.h describes, and the image an ordinary plan builds
    by enable_i8 + enable_w2 (under TCSC_PATH=mfma);
  * the GEMM: numpy on the exact integer sums (every |S| asserted below 2^24, so floating point holds them exactly)
    through the float32 formula Y = act(fl(fl(float32(S)) * s) + b), and the ordinary plan's k_gemm8 output under
    TCSC_DECODE=0.

Shapes are the smallest at which k_gemm8w2 can go wrong: K around the 16-byte fragment, the 64-k MFMA step, the 128-k
block of X8, the 256-k image block and odd counts of 128-k blocks (the last image block then has no second half of X8
behind it); N around the 16-column tile and the 128-, 256- and 512-column workgroup tiles; M around the 64- and
128-row tiles.  M <= 200 runs the 64 x 256 and the 128 x 128 workgroup shapes; the 128 x 512 one is taken from
32768 rows on (128 tiles of 256 x 256), so one test has that many rows of a narrow N."""
import numpy as np
import pytest

import tcsc_amd

pytestmark = pytest.mark.gpu

A = 0.25  # exact on integers
VARIANTS = ("basic", "optimized", "prelu_basic", "prelu_separate", "prelu_onthego", "sparse_gemm")
PRELU = ("prelu_basic", "prelu_separate", "prelu_onthego")
KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_DECODE", "TCSC_W2GEMM", "TCSC_ORDER")
MS = (17, 33, 64, 65, 128, 129, 200)
KS = (16, 64, 127, 128, 129, 256, 257, 300, 384, 2048 + 129)
NS = (1, 16, 17, 255, 256, 257, 513)
MAXM = 200


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    import torch

    return torch


@pytest.fixture
def env(monkeypatch):
    """env(TCSC_PATH=..., ...): the knobs for plans and calls made from now on; every other knob unset."""

    def set_env(**kw):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            if v is not None:
                monkeypatch.setenv(k, str(v))
        tcsc_amd.cache_clear()

    set_env()
    yield set_env
    tcsc_amd.cache_clear()


# ---- helpers ----------------------------------------------------------------------------------------------------------

def ternary(K, N, density, seed):
    rng = np.random.default_rng(seed)
    W = rng.choice(np.array([-1.0, 1.0], np.float32), (K, N))
    W[rng.random((K, N)) >= density] = 0.0
    return W


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


def dev_i32(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(torch.device("cuda:0"))


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
    """S = q . W as int64.  128 K < 2^24 bounds every partial sum, so an fp32 product holds them exactly (fp64 for a
    longer K); |S| < 2^24 is asserted either way."""
    t = np.float32 if 128 * Xq.shape[1] < 2 ** 24 else np.float64
    S = Xq.astype(t) @ Wd.astype(t)
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


def case(K, N, rows=MAXM, density=0.67):
    """W, a full-range int8 X of `rows` rows (a row of all -128, a run of 127), integer and float biases, power-of-two
    and float row scales and the exact sums: computed once per shape and left unchanged.  A test of M rows uses the
    first M."""
    key = (K, N, rows, density)
    if key not in _cases:
        seed = 18000 + 3 * K + 5 * N + rows
        rng = np.random.default_rng(seed)
        Wd = ternary(K, N, density, seed + 1)
        Xq = rng.integers(-128, 128, (rows, K), dtype=np.int64).astype(np.int8)
        Xq[2, :] = -128
        Xq[min(18, rows - 1), : K // 2 + 1] = 127
        Bi = rng.integers(-512, 513, N).astype(np.float32)
        Bf = rng.uniform(-1, 1, N).astype(np.float32)
        s2 = np.float32(2.0) ** rng.integers(-6, 4, rows).astype(np.float32)
        sf = (rng.uniform(0, 1, rows) * 0.05 + 1e-3).astype(np.float32)
        _cases[key] = dict(Wd=Wd, Xq=Xq, Bi=Bi, Bf=Bf, s2=s2, sf=sf, S=int_sums(Xq, Wd))
    return _cases[key]


def w2_image(Wd):
    """The layout of include/tcsc_gpu.h restated: tiles of 16 columns x 256 k, column-tile major then k block; lane l
    owns column 16 t + (l & 15) and the k quarter l >> 4; dword i of its 16 bytes holds the weights k = 256 kb + 64 i +
    16 (l >> 4) + j, code c = w + 1 of weight j at bit 8 (j & 3) + 2 (j >> 2); padding holds c = 1."""
    K, N = Wd.shape
    nt, nkb = (N + 15) // 16, (K + 255) // 256
    img = np.zeros((nt, nkb, 64, 4), np.uint32)
    Wp = np.zeros((nkb * 256, nt * 16), np.int64)
    Wp[:K, :N] = Wd
    for t in range(nt):
        for kb in range(nkb):
            for l in range(64):
                for i in range(4):
                    k0 = 256 * kb + 64 * i + 16 * (l >> 4)
                    p = 0
                    for j in range(16):
                        p |= int(Wp[k0 + j, 16 * t + (l & 15)] + 1) << (8 * (j & 3) + 2 * (j >> 2))
                    img[t, kb, l, i] = p
    return img.reshape(-1)


def copy_image(torch, plan, K, nc):
    nbytes = tcsc_amd.w2_image_bytes(K, nc)
    dst = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=torch.device("cuda:0"))
    plan.copy_w2(dst)
    torch.cuda.synchronize()
    return dst.cpu().numpy().view(np.uint32)


def packed_plan(W, K, c0=0, c1=None):
    """A packed plan, with what must hold straight after creation."""
    plan = tcsc_amd.Plan.packed(W, c0, c1)
    inf = plan.info()
    nc = (W.cols if c1 is None else c1) - c0
    assert plan.is_packed and plan.has_w2 and not plan.has_i8
    assert inf["device_bytes"] == tcsc_amd.w2_image_bytes(K, nc)
    assert (inf["rows"], inf["cols"], inf["col_begin"], inf["mfma_min_M"]) == (K, nc, c0, 17)
    return plan


def ordinary_plan(env, W, c0=0, c1=None, max_M=MAXM, w2=True, **knobs):
    """The parent's path: a plan with the bf16, int8 and (w2) 2-bit images, made under TCSC_PATH=mfma."""
    env(TCSC_PATH="mfma", **knobs)
    plan = tcsc_amd.Plan(W, c0, c1)
    plan.reserve(max_M)
    plan.enable_i8()
    if w2 and plan.has_i8:
        plan.enable_w2()
    return plan


# ---- 1. the image -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 15, 16, 17, 255, 256, 257, 300])
def test_image_equals_the_layout_and_the_chain(gpu, env, K):
    torch = gpu
    for N in (1, 15, 16, 17, 33):
        Wd = ternary(K, N, 0.67, 18100 + 7 * K + N)
        W = tcsc_amd.TcscMatrix.from_dense(Wd)
        env()
        plan = packed_plan(W, K)
        assert plan.info()["nnz"] == int(np.count_nonzero(Wd))
        assert plan.info()["n_pos"] == int((Wd > 0).sum()) and plan.info()["n_neg"] == int((Wd < 0).sum())
        got = copy_image(torch, plan, K, N)
        np.testing.assert_array_equal(got, w2_image(Wd), err_msg=f"layout K={K} N={N}")
        # enable_i8 / enable_w2 return OK and change nothing
        assert plan.enable_i8() is False and plan.enable_w2() is True
        assert plan.info()["device_bytes"] == tcsc_amd.w2_image_bytes(K, N)
        plan.destroy()
        chain = ordinary_plan(env, W)
        # a narrow plan of long columns drops its CSC copy and with it the images (build_csc's padding rule)
        assert chain.has_w2 or N < 16 or K > 64, (K, N)
        if chain.has_w2:
            assert not chain.is_packed
            np.testing.assert_array_equal(got, copy_image(torch, chain, K, N), err_msg=f"chain K={K} N={N}")
        chain.destroy()
        W.free()


def test_image_of_a_column_shard_and_from_device_arrays(gpu, env):
    torch = gpu
    K, N, c0, c1 = 300, 77, 5, 60
    Wd = ternary(K, N, 0.67, 18200)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = packed_plan(W, K, c0, c1)
    want = w2_image(Wd[:, c0:c1])
    got = copy_image(torch, plan, K, c1 - c0)
    np.testing.assert_array_equal(got, want)
    chain = ordinary_plan(env, W, c0, c1)
    assert chain.has_w2
    np.testing.assert_array_equal(got, copy_image(torch, chain, K, c1 - c0))
    env()
    arrs = [dev_i32(torch, a) for a in W.arrays()]
    dplan = tcsc_amd.Plan.packed_from_device(K, N, *arrs, col_begin=c0, col_end=c1)
    assert dplan.is_packed and dplan.info()["device_bytes"] == tcsc_amd.w2_image_bytes(K, c1 - c0)
    assert dplan.info()["col_begin"] == c0 and dplan.info()["nnz"] == int(np.count_nonzero(Wd[:, c0:c1]))
    np.testing.assert_array_equal(copy_image(torch, dplan, K, c1 - c0), want)
    # copy_w2 with a wrong size, and on a plan without the image
    with pytest.raises(tcsc_amd.TcscError, match="copy_w2"):
        plan.copy_w2(torch.zeros(8, dtype=torch.int32, device="cuda:0"))
    env(TCSC_PATH="gather")
    bare = tcsc_amd.Plan(W)
    with pytest.raises(tcsc_amd.TcscError, match="no 2-bit image"):
        bare.copy_w2(torch.zeros(want.size, dtype=torch.int32, device="cuda:0"))
    for p in (plan, chain, dplan, bare):
        p.destroy()
    W.free()


def hand_built(Wd, rng=None, extra_pos=(), extra_neg=()):
    """TCSC arrays of Wd with entries added per column (extra_*: (row, col) pairs) and, with rng, every column's rows
    shuffled."""
    K, N = Wd.shape
    cols_p = [list(np.nonzero(Wd[:, j] > 0)[0]) for j in range(N)]
    cols_n = [list(np.nonzero(Wd[:, j] < 0)[0]) for j in range(N)]
    for r, j in extra_pos:
        cols_p[j].append(r)
    for r, j in extra_neg:
        cols_n[j].append(r)
    if rng is not None:
        for c in cols_p + cols_n:
            rng.shuffle(c)
    csp = np.concatenate([[0], np.cumsum([len(c) for c in cols_p])]).astype(np.int32)
    csn = np.concatenate([[0], np.cumsum([len(c) for c in cols_n])]).astype(np.int32)
    rip = np.array([r for c in cols_p for r in c], np.int32)
    rin = np.array([r for c in cols_n for r in c], np.int32)
    return csp, csn, rip, rin


def test_unsorted_columns_and_a_cancelling_pair(gpu, env):
    torch = gpu
    K, N = 300, 40
    Wd = ternary(K, N, 0.67, 18300)
    Wd[7, 3] = 0.0
    Wd[299, 39] = 0.0
    # rows shuffled inside every column; (7, 3) and (299, 39) listed as +1 and as -1: weight 0
    arrs = hand_built(Wd, np.random.default_rng(18301), extra_pos=[(7, 3), (299, 39)], extra_neg=[(7, 3), (299, 39)])
    W = tcsc_amd.TcscMatrix.from_arrays(K, N, *arrs)
    plan = packed_plan(W, K)
    assert plan.info()["nnz"] == int(np.count_nonzero(Wd)) + 4  # entries, as every plan counts them
    got = copy_image(torch, plan, K, N)
    np.testing.assert_array_equal(got, w2_image(Wd))
    dplan = tcsc_amd.Plan.packed_from_device(K, N, *[dev_i32(torch, a) for a in arrs])
    np.testing.assert_array_equal(copy_image(torch, dplan, K, N), got)
    chain = ordinary_plan(env, W)
    assert chain.has_w2
    np.testing.assert_array_equal(copy_image(torch, chain, K, N), got)
    for p in (plan, dplan, chain):
        p.destroy()
    W.free()


def test_a_w_that_is_not_ternary_fails_the_build(gpu, env):
    torch = gpu
    K, N = 300, 40
    Wd = ternary(K, N, 0.67, 18400)
    Wd[5, 0] = 1.0
    arrs = hand_built(Wd, extra_pos=[(5, 0)])  # row 5 of column 0 twice as +1
    W = tcsc_amd.TcscMatrix.from_arrays(K, N, *arrs)
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*not ternary"):
        tcsc_amd.Plan.packed(W)
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*not ternary"):
        tcsc_amd.Plan.packed_from_device(K, N, *[dev_i32(torch, a) for a in arrs])
    tcsc_amd.Plan.packed(W, 1, N).destroy()  # the other columns are fine
    W.free()
    # a row outside [0, K) in device arrays
    bad = [a.copy() for a in hand_built(Wd)]
    bad[2][3] = K
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)"):
        tcsc_amd.Plan.packed_from_device(K, N, *[dev_i32(torch, a) for a in bad])
    # the reference order has no packed form
    ok = tcsc_amd.TcscMatrix.from_dense(Wd)
    tcsc_amd.set_order("reference")
    try:
        with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*reference"):
            tcsc_amd.Plan.packed(ok)
    finally:
        tcsc_amd.set_order("fast")
    ok.free()


# ---- 2. the GEMM's bits -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_gemm_bits_over_the_shape_grid(gpu, env, K):
    """Every (M, N) of the grid at this K: float scales and a float bias, bit-equal to the formula and to k_gemm8 on
    the ordinary plan."""
    torch = gpu
    for N in NS:
        c = case(K, N)
        W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
        env()
        plan = packed_plan(W, K)
        plan.reserve(MAXM)
        other = ordinary_plan(env, W, w2=False, TCSC_DECODE="0")
        # a narrow plan of long columns drops its CSC copy and with it the images (build_csc's padding rule): the
        # formula alone judges those
        assert other.has_i8 or N < 64, (K, N)
        Bf = dev_f32(torch, c["Bf"])
        for M in MS:
            path, slices = plan.launch_info_i8(M)
            assert path == "mfma", (K, N, M, path)
            Xq, Sf = dev_i8(torch, c["Xq"][:M]), dev_f32(torch, c["sf"][:M])
            got = call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2)
            assert_same_bits(got, formula(c["S"][:M], c["sf"][:M], c["Bf"], "prelu_basic", a=0.2),
                             f"formula K={K} N={N} M={M} slices={slices}")
            if other.has_i8:
                assert other.launch_info_i8(M) == ("mfma", slices), (K, N, M)
                assert_same_bits(got, call8(torch, other, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2),
                                 f"k_gemm8 K={K} N={N} M={M}")
        plan.destroy()
        other.destroy()
        W.free()


@pytest.mark.parametrize("M", [17, 65, 200])
def test_variants_scales_pitch_and_alignment(gpu, env, M):
    torch = gpu
    K, N = 300, 257
    c = case(K, N)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = packed_plan(W, K)
    Xq = dev_i8(torch, c["Xq"][:M])
    assert (c["Xq"][2] == -128).all()
    Bi, Bf = dev_f32(torch, c["Bi"]), dev_f32(torch, c["Bf"])
    S2, Sf = dev_f32(torch, c["s2"][:M]), dev_f32(torch, c["sf"][:M])
    S = c["S"][:M]
    assert np.abs(S + c["Bi"].astype(np.int64)).max() < 2 ** 24  # exact in fp32
    for variant in VARIANTS:
        # integers: scale NULL and powers of two, PReLU with a = 0.25 -- exact
        np.testing.assert_array_equal(call8(torch, plan, Xq, None, Bi, M, N, variant),
                                      formula(S, None, c["Bi"], variant), err_msg=f"{variant}/s=NULL")
        np.testing.assert_array_equal(call8(torch, plan, Xq, S2, Bi, M, N, variant),
                                      formula(S, c["s2"][:M], c["Bi"], variant), err_msg=f"{variant}/s=2^e")
        # arbitrary fp32 scales and a float bias: the multiply and the add are rounded apart
        assert_same_bits(call8(torch, plan, Xq, Sf, Bf, M, N, variant, a=0.2),
                         formula(S, c["sf"][:M], c["Bf"], variant, a=0.2), f"{variant}/float")
    want = formula(S, c["sf"][:M], c["Bf"], "prelu_basic", a=0.2)
    # ldy > N, a multiple of 4 and not: the sentinel columns stay (call8 checks them)
    for ldy in (N + 3, N + 6):
        assert_same_bits(call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", ldy, a=0.2), want, f"pitch {ldy}")
    # X one byte into its allocation: k_pack8's byte form
    Xu = dev_i8(torch, c["Xq"][:M], offset=1)
    assert Xu.data_ptr() % 16 == 1
    assert_same_bits(call8(torch, plan, Xu, Sf, Bf, M, N, "prelu_basic", a=0.2), want, "unaligned")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("w", [1, -1, 0])
def test_extremes(gpu, env, w):
    """W all +1, all -1 or all zero against q all -128 and all 127: the largest sums, and the signed bytes of all
    three codes in every position."""
    torch = gpu
    K, N, M = 2048 + 129, 48, 33
    Wd = np.full((K, N), w, np.float32)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = packed_plan(W, K)
    Bi = dev_f32(torch, np.arange(N, dtype=np.float32) - 20)
    for q in (-128, 127):
        Xq = np.full((M, K), q, np.int8)
        S = np.full((M, N), q * w * K, np.int64)
        Y = call8(torch, plan, dev_i8(torch, Xq), None, Bi, M, N, "prelu_basic")
        np.testing.assert_array_equal(Y, formula(S, None, np.arange(N) - 20, "prelu_basic"), err_msg=f"w={w} q={q}")
    plan.destroy()
    W.free()


# the int8 rule gives a slice at least four 128-k blocks, so K = 2048 + 129 (18 blocks) splits 4 ways at the most; 16
# slices are forced at K = 10012 (79 blocks, an odd count again).  Narrow tiles (M = 33: 2 workgroups unsplit) and
# 128 x 128 ones (M = 129: 6).
@pytest.mark.parametrize("K,M,wgs,slices", [(2177, 33, 4, 2), (2177, 33, 6, 3), (2177, 33, 8, 4), (10012, 33, 32, 16),
                                            (2177, 129, 12, 2), (2177, 129, 18, 3), (10012, 129, 96, 16)])
def test_split_k_gives_the_same_bits(gpu, env, K, M, wgs, slices):
    torch = gpu
    N = 257
    c = case(K, N, rows=129)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    env(TCSC_MFMA_WGS="0")
    plan = packed_plan(W, K)
    assert plan.launch_info_i8(M) == ("mfma", 1)
    Xq, Sf, Bf = dev_i8(torch, c["Xq"][:M]), dev_f32(torch, c["sf"][:M]), dev_f32(torch, c["Bf"])
    want = formula(c["S"][:M], c["sf"][:M], c["Bf"], "prelu_basic", a=0.2)
    unsplit = call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2)
    assert_same_bits(unsplit, want, "unsplit")
    env(TCSC_MFMA_WGS=wgs)
    assert plan.launch_info_i8(M) == ("mfma", slices)
    need, _ = plan.workspace(M, "mfma")
    assert need >= slices * M * N * 4
    for variant, ldy in (("prelu_basic", N), ("sparse_gemm", N + 3)):
        got = call8(torch, plan, Xq, Sf, Bf, M, N, variant, ldy, a=0.2)
        assert_same_bits(got, formula(c["S"][:M], c["sf"][:M], c["Bf"], variant, a=0.2), f"{slices} slices {variant}")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("K,wgs,slices", [(300, None, 1), (1025, 1028, 2)])
def test_the_128x512_tiles(gpu, env, K, wgs, slices):
    """32768 + 5 rows of a 17-column plan are 129 x 1 tiles of 256 x 256: the 8-wave 128 x 512 shape, with a ragged
    last row tile and one column tile in 32; unsplit, and with K split over two slices."""
    torch = gpu
    M, N = 32768 + 5, 17
    c = case(K, N, rows=M)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    env(TCSC_MFMA_WGS=wgs)
    plan = packed_plan(W, K)
    assert plan.launch_info_i8(M) == ("mfma", slices)
    other = ordinary_plan(env, W, max_M=M, w2=False, TCSC_DECODE="0", TCSC_MFMA_WGS=wgs)
    assert other.launch_info_i8(M) == ("mfma", slices)
    Xq, Sf, Bf = dev_i8(torch, c["Xq"]), dev_f32(torch, c["sf"]), dev_f32(torch, c["Bf"])
    got = call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2)
    assert_same_bits(got, formula(c["S"], c["sf"], c["Bf"], "prelu_basic", a=0.2), "formula")
    assert_same_bits(got, call8(torch, other, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2), "k_gemm8")
    plan.destroy()
    other.destroy()
    W.free()


def test_more_than_2_22_rows_run_in_pieces(gpu, env):
    """2^22 + 17 rows: one launch of 2^22 rows and one of 17 on one workspace."""
    torch = gpu
    M, K, N = (1 << 22) + 17, 16, 3
    rng = np.random.default_rng(18500)
    Wd = ternary(K, N, 0.67, 18501)
    Xq = rng.integers(-128, 128, (M, K), dtype=np.int8)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = packed_plan(W, K)
    plan.reserve(M)
    held = plan.info()["device_bytes"]
    need, reserved = plan.workspace(M)
    assert 0 < need <= reserved
    Bi = np.array([1.0, -2.0, 3.0], np.float32)
    Y = call8(torch, plan, dev_i8(torch, Xq), None, dev_f32(torch, Bi), M, N, "prelu_basic")
    np.testing.assert_array_equal(Y, formula(int_sums(Xq, Wd), None, Bi, "prelu_basic"))
    assert plan.info()["device_bytes"] == held
    plan.destroy()
    W.free()


# ---- 3. the knob on an ordinary plan ----------------------------------------------------------------------------------

@pytest.mark.parametrize("K,N", [(300, 257), (2177, 513), (129, 17)])
def test_w2gemm_knob_on_an_ordinary_plan(gpu, env, K, N):
    torch = gpu
    c = case(K, N)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = ordinary_plan(env, W, TCSC_DECODE="0")
    assert plan.has_i8 and plan.has_w2 and not plan.is_packed
    held = plan.info()["device_bytes"]
    Bf = dev_f32(torch, c["Bf"])
    for wgs in (None, 8):
        for M in MS:
            Xq, Sf = dev_i8(torch, c["Xq"][:M]), dev_f32(torch, c["sf"][:M])
            env(TCSC_PATH="mfma", TCSC_DECODE="0", TCSC_MFMA_WGS=wgs)
            route = plan.launch_info_i8(M)
            base = call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2)
            for knob in ("0", "1"):
                env(TCSC_PATH="mfma", TCSC_DECODE="0", TCSC_MFMA_WGS=wgs, TCSC_W2GEMM=knob)
                assert plan.launch_info_i8(M) == route and route[0] == "mfma"
                assert plan.workspace(M)[0] <= plan.workspace(M)[1]
                assert_same_bits(call8(torch, plan, Xq, Sf, Bf, M, N, "prelu_basic", a=0.2), base,
                                 f"TCSC_W2GEMM={knob} K={K} N={N} M={M} route={route}")
            assert_same_bits(base, formula(c["S"][:M], c["sf"][:M], c["Bf"], "prelu_basic", a=0.2), "formula")
    assert plan.info()["device_bytes"] == held
    plan.destroy()
    W.free()


# ---- 4. routing, workspace, capture, refusals -------------------------------------------------------------------------

def test_up_to_16_rows_decode_whatever_the_knobs_say(gpu, env):
    torch = gpu
    K, N = 300, 257
    c = case(K, N)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = packed_plan(W, K)
    Bf = dev_f32(torch, c["Bf"])
    for knobs in ({}, {"TCSC_DECODE": "0"}, {"TCSC_PATH": "gather", "TCSC_DECODE": "0", "TCSC_SMALL_M": "4"}):
        env(**knobs)
        for M in (1, 4, 5, 16):
            assert plan.launch_info_i8(M) == ("decode", 1), (knobs, M)
            assert plan.workspace(M)[0] == 0
            got = call8(torch, plan, dev_i8(torch, c["Xq"][:M]), dev_f32(torch, c["sf"][:M]), Bf, M, N, "prelu_basic",
                        a=0.2)
            assert_same_bits(got, formula(c["S"][:M], c["sf"][:M], c["Bf"], "prelu_basic", a=0.2), f"{knobs} M={M}")
        assert plan.launch_info_i8(17)[0] == "mfma"
    assert plan.info()["device_bytes"] == tcsc_amd.w2_image_bytes(K, N)  # the decode path needs no workspace
    plan.destroy()
    W.free()


def test_reserve_then_calls_allocate_nothing_and_can_be_captured(gpu, env):
    torch = gpu
    K, N = 2177, 257
    c = case(K, N)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = packed_plan(W, K)
    plan.reserve(200)
    held = plan.info()["device_bytes"]
    assert held > tcsc_amd.w2_image_bytes(K, N)
    for M in range(1, 201):
        need, reserved = plan.workspace(M)
        assert need <= reserved, M
        assert plan.workspace(M, "mfma")[0] <= reserved and plan.workspace(M, "decode")[0] == 0
    dev = torch.device("cuda:0")
    Bf = dev_f32(torch, c["Bf"])
    side = torch.cuda.Stream()
    for M in (1, 16, 17, 64, 200):
        Qg = torch.zeros((M, K), dtype=torch.int8, device=dev)
        Sg = torch.zeros(M, device=dev)
        Yg = torch.empty((M, N), device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            plan.sgemm_i8(Qg, Sg, Bf, Yg, M, N, "prelu_basic", 0.2, torch.cuda.current_stream().cuda_stream)
        for r0 in (0, MAXM - M):
            Qg.copy_(dev_i8(torch, c["Xq"][r0:r0 + M]))
            Sg.copy_(dev_f32(torch, c["sf"][r0:r0 + M]))
            Yg.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_same_bits(Yg.cpu().numpy(),
                             formula(c["S"][r0:r0 + M], c["sf"][r0:r0 + M], c["Bf"], "prelu_basic", a=0.2),
                             f"replay M={M} rows from {r0}")
        del g
        assert plan.info()["device_bytes"] == held, M
    plan.destroy()
    W.free()


def test_calls_that_need_another_format_are_refused(gpu, env):
    torch = gpu
    K, N, M = 64, 32, 4
    W = tcsc_amd.TcscMatrix.from_dense(ternary(K, N, 0.67, 18600))
    plan = packed_plan(W, K)
    dev = torch.device("cuda:0")
    X = torch.zeros((M, K), device=dev)
    Xb = torch.zeros((M, K), dtype=torch.bfloat16, device=dev)
    B, Y = torch.zeros(N, device=dev), torch.zeros((M, N), device=dev)
    calls = {
        "tcsc_gpu_sgemm": lambda: plan.sgemm(X, B, Y, M, N),
        "tcsc_gpu_sgemm_bf16": lambda: plan.sgemm_bf16(Xb, B, Y, M, N),
        "tcsc_gpu_prepare_x": lambda: plan.prepare_x(X, M),
        "tcsc_gpu_sgemm_prepared": lambda: plan.sgemm_prepared(B, Y, M, N),
        "tcsc_gpu_sgemm_t": lambda: plan.sgemm_t(Y, X, M, K),
        "tcsc_gpu_launch_info": lambda: plan.launch_info(M),
        "tcsc_gpu_launch_info_bf16": lambda: plan.launch_info_bf16(M),
        "tcsc_gpu_launch_geometry": lambda: plan.launch_geometry(M),
        "tcsc_gpu_launch_combine": lambda: plan.combine_mode(M),
    }
    for name, call in calls.items():
        with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)") as e:
            call()
        assert "packed plan" in tcsc_amd.last_error() and name + ":" in tcsc_amd.last_error(), (name, str(e.value))
    assert plan.info()["device_bytes"] == tcsc_amd.w2_image_bytes(K, N)  # nothing was allocated on the way
    plan.destroy()
    W.free()


# ---- 5. the layer -----------------------------------------------------------------------------------------------------

def test_packed_layer_equals_forward_int8(gpu, env):
    torch = gpu
    from tcsc_amd.nn import PackedTernaryLinear, TernaryLinear

    K, N = 300, 130
    c = case(K, N)
    X = np.random.default_rng(18700).uniform(-1, 1, (40, K)).astype(np.float32)
    env(TCSC_PATH="mfma")  # the yardstick is k_gemm8 at both row counts: by default 3 rows would take the small-M path
    plain = TernaryLinear(c["Wd"], bias=c["Bf"], a=0.2)
    plain.reserve(40, int8=True)
    assert plain.plan.has_i8 and not plain.plan.has_w2
    layer = PackedTernaryLinear(c["Wd"], bias=c["Bf"], a=0.2)
    layer.reserve(40)
    assert layer.plan.is_packed and not list(layer.parameters())
    held = layer.plan.info()["device_bytes"]
    for rows in (3, 40):
        x = dev_f32(torch, X[:rows])
        with torch.no_grad():
            y = layer(x)
            y0 = plain.forward_int8(x)
        torch.cuda.synchronize()
        assert plain.plan.launch_info_i8(rows)[0] == "mfma"
        assert layer.plan.launch_info_i8(rows)[0] == ("decode" if rows <= 16 else "mfma")
        assert_same_bits(y.cpu().numpy(), y0.cpu().numpy(), f"rows={rows}")
    assert layer.plan.info()["device_bytes"] == held
    with pytest.raises(tcsc_amd.TcscError, match="inference only"):
        layer(dev_f32(torch, X[:3]).requires_grad_())
    # identity activation, leading dimensions
    ident = PackedTernaryLinear(c["Wd"], a=None)
    y = ident(dev_f32(torch, X[:6]).reshape(2, 3, K))
    assert y.shape == (2, 3, N)
