"""int8 decode up to 64 rows: tcsc_gpu_sgemm_i8 calls of 17 .. 64 rows on the row-tiled k_decode8r,
taken where tcsc_gpu_plan_set_decode_rows admits them.

The contract is an equality of bits, and the yardsticks are those of tests/test_gpu_decode.py, restated here, neither
of them the row-tiled launch itself:
  (a) numpy: the exact integer sums (every |S| asserted below 2^24, so fp64 holds them) through the float32 formula
      Y = act(fl(fl(fl(float32(S)) * s) * c) + b), then fl(v + r) for a residual and the rounding to bf16 restated
      on the bits;
  (b) the same call on the same plan with the setting at 16: the k_gemm8w2 / k_gemm8 route.
Every case first asserts that launch_info_i8 names `decode` with the setting on and `mfma` with it off.  Y is
compared as integer bits over its whole sentinel-filled allocation, rows beyond M included.

X is full-range int8; in every 16-row tile one row is all -128 and two carry a run of 127, and so does the last live
row of each M.  Shapes are the smallest at which the kernel can go wrong: K around the 16-byte fragment, the 64-k
step, the 256-k block and the 8 waves' round, N around the 16-column tile, and the widths at which the launcher picks
each (row tiles, column tiles) pair on the chip's CU count."""
import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

A = 0.2
PRELU = pyoracle.PRELU_VARIANTS
VARIANTS = ("prelu_basic", "basic", "sparse_gemm", "prelu_onthego", "optimized", "prelu_separate")
KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")
MS = (17, 31, 32, 33, 47, 48, 49, 63, 64)
KS = (1, 15, 16, 17, 63, 65, 255, 256, 257, 2047, 2048, 2049, 2304, 4352)
PAIRS = {(2, 1), (2, 2), (2, 4), (4, 1), (4, 2)}  # (row tiles, column tiles) of DESIGN.md §27
SENT = 7.0
DEV = "cuda:0"
ROWS = 64


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    lib = tcsc_amd.lib()
    for name in ("tcsc_gpu_plan_set_decode_rows", "tcsc_gpu_launch_info_decode"):  # without the feature: fails here
        assert getattr(lib, name) is not None
    import torch

    return torch


@pytest.fixture
def env(monkeypatch):
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

def int_sums(q, Wd):
    S = q.astype(np.float64) @ Wd.astype(np.float64)
    assert np.abs(S).max(initial=0) < 2 ** 24 and np.array_equal(S, np.rint(S))
    return S.astype(np.int64)


def np_bf16_bits(v):
    """Round to nearest even on the fp32 bits (finite inputs)."""
    v = np.ascontiguousarray(v, np.float32)
    assert np.isfinite(v).all()
    u = v.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_values(v):
    return (np_bf16_bits(v).astype(np.uint32) << 16).view(np.float32)


def formula(S, s, c, b, variant, ytype, a=A, r=None):
    """The bits of Y (uint32 for an fp32 Y, uint16 for a bf16 one); s or c None: ones; r: the residual's values."""
    v = S.astype(np.float32)
    if s is not None:
        v = v * np.asarray(s, np.float32)[:, None]
    if c is not None:
        v = v * np.asarray(c, np.float32)[None, :]
    v = v + np.asarray(b, np.float32)[None, :]
    if variant in PRELU:
        v = np.where(v < 0, np.float32(a) * v, v)
    if r is not None:
        v = v + np.asarray(r, np.float32)
    assert v.dtype == np.float32
    return np_bf16_bits(v) if ytype == "bf16" else np.ascontiguousarray(v).view(np.uint32)


_cases = {}


def case(o, K, N, density=0.67):
    """W, 64 full-range int8 rows (in every 16-row tile: row 2 all -128, rows 0 and 15 with a run of 127), an integer
    and a float bias, power-of-two and float row scales, column scales -- computed once per shape and left unchanged."""
    key = (K, N, density)
    if key not in _cases:
        seed = 27000 + 3 * K + 5 * N
        rng = np.random.default_rng(seed)
        Wd = o.ternary((K, N), density, seed)
        Xq = rng.integers(-128, 128, (ROWS, K), dtype=np.int64).astype(np.int8)
        for t in range(ROWS // 16):
            Xq[16 * t + 2, :] = -128
            Xq[16 * t, : K // 2 + 1] = 127
            Xq[16 * t + 15, K // 3:] = 127
        pool = np.array([1.0, 0.5, 0.0123, -1.75, 0.0, 3.0, 0.3, -0.0625], np.float32)
        Cs = pool[rng.integers(0, pool.size, N)]
        Cs[:min(N, 5)] = pool[:min(N, 5)]
        _cases[key] = dict(K=K, N=N, Wd=Wd, Xq=Xq, Bi=o.integers((N,), seed + 2), Bf=o.uniform((N,), seed + 3),
                           s2=np.float32(2.0) ** rng.integers(-6, 4, ROWS).astype(np.float32),
                           sf=(np.abs(o.uniform((ROWS,), seed + 4)) * np.float32(0.05) + np.float32(1e-3)).astype(np.float32),
                           Cs=Cs.astype(np.float32), rows={})
    return _cases[key]


def rows_of(c, M):
    """(X, S) of a call of M rows: the case's first M rows with a run of 127 in the last live one, and their sums."""
    if M not in c["rows"]:
        X = c["Xq"][:M].copy()
        X[M - 1, : c["K"] // 3 + 1] = 127
        c["rows"][M] = (X, int_sums(X, c["Wd"]))
    return c["rows"][M]


# ---- device buffers ---------------------------------------------------------------------------------------------------

def dev_f32(torch, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def dev_i8(torch, q, offset=0):
    """A contiguous torch.int8 device tensor with these values, `offset` bytes into its allocation."""
    buf = torch.zeros(q.size + 32, dtype=torch.int8, device=DEV)
    v = buf[offset:offset + q.size].view(*q.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(q, np.int8)).to(DEV))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() == buf.data_ptr() + offset
    return v


class YBuf:
    """A sentinel-filled allocation of M + 3 rows of pitch ldy; `init` (M x N float32 values): what rows < M,
    columns < N hold before the call (an in-place residual)."""

    def __init__(self, torch, M, N, ldy, ytype, init=None):
        self.torch, self.M, self.N, self.ldy, self.ytype = torch, M, N, ldy, ytype
        dt = torch.float32 if ytype == "f32" else torch.bfloat16
        self.Y = torch.full((M + 3, ldy), SENT, dtype=dt, device=DEV)
        if init is not None:
            self.Y[:M, :N] = torch.from_numpy(np.ascontiguousarray(init, np.float32)).to(DEV).to(dt)

    def bits(self):
        self.torch.cuda.synchronize()
        if self.ytype == "f32":
            return self.Y.cpu().numpy().view(np.uint32)
        return self.Y.view(self.torch.int16).cpu().numpy().view(np.uint16)

    def check(self, ybits, what):
        sent = np.float32(SENT).view(np.uint32)
        want = np.full((self.M + 3, self.ldy), sent if self.ytype == "f32" else sent >> 16, ybits.dtype)
        want[:self.M, :self.N] = ybits
        got = self.bits()
        bad = np.argwhere(got != want)
        if bad.size:
            r, col = bad[0]
            raise AssertionError(f"{what}: {len(bad)} elements differ, the first at row {r} column {col} (M={self.M} "
                                 f"N={self.N} ldy={self.ldy}): got {int(got[r, col]):#x}, expected {int(want[r, col]):#x}")


def run(torch, plan, X, s, cs, b, M, N, ytype="f32", variant="prelu_basic", a=A, ldy=None, R=None, inplace=False):
    """One sgemm_i8 of M rows; R: the residual's values (M x N), in its own buffer or, inplace, in Y's."""
    ldy = ldy or N
    Xd = X if hasattr(X, "data_ptr") else dev_i8(torch, X)
    yb = YBuf(torch, M, N, ldy, ytype, init=R if inplace else None)
    if R is None:
        plan.sgemm_i8(Xd, dev_f32(torch, s), dev_f32(torch, b), yb.Y, M, ldy, variant, a, col_scale=dev_f32(torch, cs))
    elif inplace:
        plan.sgemm_i8(Xd, dev_f32(torch, s), dev_f32(torch, b), yb.Y, M, ldy, "basic", 0.0, col_scale=dev_f32(torch, cs),
                      residual=yb.Y, ldr=ldy)
    else:
        rb = YBuf(torch, M, N, N + 2, ytype, init=R)
        before = rb.bits().copy()
        plan.sgemm_i8(Xd, dev_f32(torch, s), dev_f32(torch, b), yb.Y, M, ldy, "basic", 0.0, col_scale=dev_f32(torch, cs),
                      residual=rb.Y, ldr=N + 2)
        assert np.array_equal(rb.bits(), before), "R was written"
    return yb


def on(plan, M, rows=64):
    plan.set_decode_rows(rows)
    assert plan.decode_rows == rows
    assert plan.launch_info_i8(M) == ("decode", 1), (M, plan.launch_info_i8(M))
    assert not plan.is_packed or plan.workspace(M)[0] == 0  # an ordinary plan's AUTO sizes its fp32 call
    return plan.launch_info_decode(M)[:2]


def off(plan, M):
    plan.set_decode_rows(16)
    assert plan.decode_rows == 16
    assert plan.launch_info_i8(M)[0] == "mfma", (M, plan.launch_info_i8(M))
    assert not plan.is_packed or plan.workspace(M)[0] == plan.workspace(M, "mfma")[0] > 0


def both(torch, plan, c, M, what, s="sf", cs=None, b="Bf", X=None, **kw):
    """The call on the row-tiled launch against yardstick (a) and against the same call with the setting at 16."""
    N = c["N"]
    Xm, S = rows_of(c, M)
    sv = None if s is None else c[s][:M]
    csv = None if cs is None else c[cs]
    want = formula(S, sv, csv, c[b], kw.get("variant", "prelu_basic") if kw.get("R") is None else "basic",
                   kw.get("ytype", "f32"), kw.get("a", A), kw.get("R"))
    pair = on(plan, M)
    run(torch, plan, Xm if X is None else X, sv, csv, c[b], M, N, **kw).check(want, f"{what} M={M}: decode")
    off(plan, M)
    run(torch, plan, Xm if X is None else X, sv, csv, c[b], M, N, **kw).check(want, f"{what} M={M}: setting 16")
    return pair


def packed(Wd, rows=ROWS + 1):
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan.packed(W)
    plan.reserve(rows)
    return W, plan


def ordinary(env, Wd, rows=ROWS + 1, **knobs):
    env(TCSC_PATH="mfma", **knobs)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan(W)
    plan.reserve(rows)
    assert plan.enable_i8() and plan.enable_w2()
    return W, plan


def r_values(M, N, ytype, seed):
    rng = np.random.default_rng(seed)
    R = (rng.standard_normal((M, N)) * rng.choice([1e-3, 1.0, 50.0], (M, N))).astype(np.float32)
    R.reshape(-1)[rng.permutation(M * N)[:2]] = np.array([0.0, -0.0], np.float32)[:min(2, M * N)]
    return bf16_values(R) if ytype == "bf16" else R


# ---- 1. rows and K ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_rows_and_k(gpu, oracle, env, K):
    """Every M at tile edges with one live row in the last tile, over K around the fragment, the step, the block and
    the waves' round; K % 16 != 0 takes the byte loads.  4352 gives wave 0 three blocks: the prefetch wraps twice."""
    torch = gpu
    env()
    c = case(oracle, K, 40)
    W, plan = packed(c["Wd"])
    for M in MS:
        rt, ct = both(torch, plan, c, M, f"K={K}")
        assert rt == (2 if M <= 32 else 4) and ct in (1, 2, 4)
    plan.set_decode_rows(64)
    assert plan.launch_info_i8(65)[0] == "mfma" and plan.launch_info_i8(16) == ("decode", 1)
    plan.destroy()
    W.free()


# ---- 2. columns and instantiations ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 15, 16, 17, 33, 130])
def test_column_edges(gpu, oracle, env, N):
    torch = gpu
    env()
    c = case(oracle, 65, N)
    W, plan = packed(c["Wd"])
    for M in (17, 33, 64):
        both(torch, plan, c, M, f"N={N}", ytype="bf16" if M == 33 else "f32", cs="Cs")
    plan.destroy()
    W.free()


def test_every_instantiation(gpu, oracle, env):
    """The widths at which launch_info_decode reports each (row tiles, column tiles) pair on this chip, each with a
    ragged last workgroup and a ragged last tile; at each pair every Y type, tail (plain, PReLU, residual) and both
    load forms (X aligned, X one byte off).  The pairs seen are exactly DESIGN's."""
    torch = gpu
    env()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    K = 272
    seen = set()
    for N in (130, 16 * (2 * cus + 1) - 8, 16 * (4 * cus + 1) - 8):
        c = case(oracle, K, N)
        W, plan = packed(c["Wd"])
        tiles = (N + 15) // 16
        for M in (24, 40):
            pair = on(plan, M)
            rt, ct, wgs = plan.launch_info_decode(M)
            assert rt * ct <= 8 and wgs == (tiles + ct - 1) // ct
            assert ct == 1 or tiles % ct != 0, "a ragged last workgroup"
            assert ct == 1 or wgs >= cus, "the grid covers the chip"
            seen.add(pair)
            Xm, _ = rows_of(c, M)
            for offset in (0, 1):
                Xd = dev_i8(torch, Xm, offset)
                for ytype in ("f32", "bf16"):
                    R = r_values(M, N, ytype, M + N)
                    assert both(torch, plan, c, M, f"N={N} {ytype} off={offset}", X=Xd, ytype=ytype) == pair
                    both(torch, plan, c, M, f"N={N} {ytype} off={offset} basic", X=Xd, ytype=ytype, variant="basic", cs="Cs")
                    both(torch, plan, c, M, f"N={N} {ytype} off={offset} res", X=Xd, ytype=ytype, R=R, inplace=bool(offset))
        plan.destroy()
        W.free()
    assert seen == PAIRS, seen


# ---- 3. the formula, bit for bit ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,N", [(333, 77), (512, 48)])
def test_bits(gpu, oracle, env, K, N):
    torch = gpu
    env()
    c = case(oracle, K, N)
    W, plan = packed(c["Wd"])
    for M in (17, 40, 64):
        _, S = rows_of(c, M)
        assert np.abs(S + c["Bi"].astype(np.int64)).max() < 2 ** 24  # exact in fp32
        for variant in VARIANTS:
            both(torch, plan, c, M, f"{variant}/s=NULL", s=None, b="Bi", variant=variant, a=0.25)
            both(torch, plan, c, M, f"{variant}/s=2^e", s="s2", b="Bi", variant=variant, a=0.25)
            both(torch, plan, c, M, f"{variant}/float", variant=variant)
        both(torch, plan, c, M, "column scales, bf16", cs="Cs", ytype="bf16")
        both(torch, plan, c, M, "column scales, bf16, no PReLU", cs="Cs", ytype="bf16", variant="basic")
        both(torch, plan, c, M, "pitch", ldy=N + 5)
        both(torch, plan, c, M, "pitch, bf16", ldy=N + 3, ytype="bf16")
        for ytype in ("f32", "bf16"):
            R = r_values(M, N, ytype, 5 * M + N)
            for inplace in (False, True):
                both(torch, plan, c, M, f"residual {ytype} inplace={inplace}", cs="Cs", ytype=ytype, R=R, inplace=inplace,
                     ldy=N + 4 if inplace else N)
    plan.destroy()
    W.free()


@pytest.mark.parametrize("K", [256, 300])
def test_x_one_byte_off(gpu, oracle, env, K):
    """K = 256 would take the 16-B loads; one byte off they may not be used.  K = 300: the byte loads either way."""
    torch = gpu
    env()
    c = case(oracle, K, 100)
    W, plan = packed(c["Wd"])
    for M in (31, 49):
        Xu = dev_i8(torch, rows_of(c, M)[0], offset=1)
        assert Xu.data_ptr() % 16 == 1
        both(torch, plan, c, M, f"K={K} unaligned", X=Xu)
    plan.destroy()
    W.free()


# ---- 4. plans and entry points ----------------------------------------------------------------------------------------------

def test_an_ordinary_plan(gpu, oracle, env):
    """After enable_w2 the setting routes as on a packed plan (setting 16: k_gemm8 on the int8 image); $TCSC_DECODE=0
    still vetoes, a pinned MFMA path still sizes the GEMM, M <= 16 is untouched."""
    torch = gpu
    K, N = 333, 77
    c = case(oracle, K, N)
    W, plan = ordinary(env, c["Wd"])
    before = [plan.launch_info_i8(M) for M in range(1, 17)]
    for M in (17, 40, 64):
        both(torch, plan, c, M, "ordinary")
        both(torch, plan, c, M, "ordinary, residual bf16", ytype="bf16", R=r_values(M, N, "bf16", M), inplace=True)
    plan.set_decode_rows(64)
    assert [plan.launch_info_i8(M) for M in range(1, 17)] == before
    assert plan.launch_info_i8(40) == ("decode", 1) and plan.launch_info_i8(65)[0] == "mfma"
    assert plan.workspace(40, "mfma")[0] > 0 and plan.workspace(40, "decode")[0] == 0
    assert all(plan.launch_info(M)[0] != "decode" and plan.launch_info_bf16(M)[0] != "decode" for M in (17, 40))
    env(TCSC_PATH="mfma", TCSC_DECODE="0")
    assert plan.launch_info_i8(40)[0] == "mfma"
    Xm, S = rows_of(c, 40)
    run(torch, plan, Xm, c["sf"][:40], None, c["Bf"], 40, N).check(
        formula(S, c["sf"][:40], None, c["Bf"], "prelu_basic", "f32"), "TCSC_DECODE=0")
    env(TCSC_PATH="mfma", TCSC_DECODE="1")
    assert plan.launch_info_i8(40) == ("decode", 1)
    plan.set_decode_rows(16)
    assert plan.launch_info_i8(40)[0] == "mfma"  # the knob forces nothing above 16 rows
    plan.destroy()
    W.free()


def np_quantize(x):
    x = np.ascontiguousarray(x, np.float32)
    amax = np.max(np.abs(x), axis=1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        live = (amax > 0) & ~np.isinf(np.float32(127.0) / amax)  # a row whose 127 / amax is inf counts as a row of zeros
        scale = np.where(live, amax / np.float32(127.0), np.float32(0)).astype(np.float32)
        inv = np.where(live, np.float32(127.0) / amax, np.float32(0)).astype(np.float32)
    r = np.rint((x * inv[:, None]).astype(np.float32))
    return np.clip(r, -127, 127).astype(np.int8), scale


@pytest.mark.parametrize("qfuse", [None, "1"])
def test_q8_calls_are_the_quantizer_then_this_kernel(gpu, oracle, env, qfuse):
    """sgemm_q8 and sgemm_q8_norm at M = 40, fp32 and bf16 x: decode, never fused (whatever $TCSC_QFUSE says), the
    bits of the same call with the setting at 16 -- and, without the norm, of the numpy quantizer and formula."""
    torch = gpu
    K, N, M = 333, 77, 40
    c = case(oracle, K, N)
    env(TCSC_QFUSE=qfuse)
    W, plan = packed(c["Wd"])
    rng = np.random.default_rng(2740)
    X32 = (rng.standard_normal((M, K)) * rng.choice([1e-3, 1.0, 37.0], (M, 1))).astype(np.float32)
    X32[2] = 0.0
    gamma = dev_f32(torch, 1.0 + 0.1 * rng.standard_normal(K))
    Bd, Cd = dev_f32(torch, c["Bf"]), dev_f32(torch, c["Cs"])
    for xt in ("f32", "bf16"):
        X = dev_f32(torch, X32) if xt == "f32" else dev_f32(torch, X32).to(torch.bfloat16)
        q, s = np_quantize(X.to(torch.float32).cpu().numpy())
        want = formula(int_sums(q, c["Wd"]), s, c["Cs"], c["Bf"], "prelu_basic", "bf16")
        got = {}
        for rows in (64, 16):
            plan.set_decode_rows(rows)
            route = ("decode", 1, False) if rows == 64 else ("mfma", plan.launch_info_i8(M)[1], False)
            assert plan.launch_info_q8(M, xt) == route and plan.launch_info_q8_norm(M, xt) == route
            assert plan.launch_info_q8(16, xt)[0] == "decode"
            for norm in (False, True):
                yb = YBuf(torch, M, N, N + 1, "bf16")
                Xq = torch.zeros((M, K), dtype=torch.int8, device=DEV)
                Sc = torch.full((M + 1,), 5.0, device=DEV)
                if norm:
                    plan.sgemm_q8_norm(X, Xq, Sc, Bd, yb.Y, M, N + 1, gamma, 1e-5, "prelu_basic", A, col_scale=Cd)
                else:
                    plan.sgemm_q8(X, Xq, Sc, Bd, yb.Y, M, N + 1, "prelu_basic", A, col_scale=Cd)
                    yb.check(want, f"q8 {xt} rows={rows}")
                    np.testing.assert_array_equal(Xq.cpu().numpy(), q)  # unfused: the quantizer wrote its scratch
                got[rows, norm] = (yb.bits().copy(), Sc.cpu().numpy())
                assert got[rows, norm][1][M] == 5.0
        for norm in (False, True):
            np.testing.assert_array_equal(got[64, norm][0], got[16, norm][0], err_msg=f"{xt} norm={norm}")
            np.testing.assert_array_equal(got[64, norm][1].view(np.uint32), got[16, norm][1].view(np.uint32))
    plan.destroy()
    W.free()


# ---- 5. workspace and capture ---------------------------------------------------------------------------------------------

def test_reserve_and_the_gated_and_grouped_calls(gpu, oracle, env):
    """reserve(64) sizes the MFMA route whatever the setting; the gated and the grouped call read no setting: at
    M = 40 on plans set to 64 they allocate nothing and give the bits they give on plans set to 16."""
    torch = gpu
    env()
    K, N, M = 333, 77, 40
    c = case(oracle, K, N)
    c2 = case(oracle, K, N, 0.5)
    plans = []
    for rows in (16, 64):
        Wa, pa = packed(c["Wd"], rows=1)
        Wb, pb = packed(c2["Wd"], rows=1)
        for p in (pa, pb):
            p.set_decode_rows(rows)
            p.reserve(64)
        plans.append((Wa, pa, Wb, pb))
    (_, a16, _, b16), (_, a64, _, b64) = plans
    assert a16.info()["device_bytes"] == a64.info()["device_bytes"] and a64.workspace(40)[1] >= a64.workspace(40, "mfma")[0] > 0
    held = [p.info()["device_bytes"] for p in (a64, b64)]
    Xm, S = rows_of(c, M)
    Xd, Sd = dev_i8(torch, Xm), dev_f32(torch, c["sf"][:M])
    Bg, Bu = dev_f32(torch, c["Bf"]), dev_f32(torch, c2["Bf"])
    out = {}
    for tag, pg, pu in (("16", a16, b16), ("64", a64, b64)):
        assert tcsc_amd.launch_info_glu(pg, pu, M)[0] == "mfma" and tcsc_amd.launch_info_group([pg, pu], M)[0] == "mfma"
        Y = torch.full((M + 1, N), SENT, device=DEV)
        G = torch.empty((M, N), device=DEV)
        tcsc_amd.sgemm_i8_glu(pg, pu, Xd, Sd, Bg, Bu, Y, M, N, "relu2", G=G)
        Y0, Y1 = torch.full((M + 1, N), SENT, device=DEV), torch.full((M + 1, N), SENT, device=DEV)
        tcsc_amd.sgemm_i8_group([pg, pu], Xd, Sd, [Bg, Bu], [Y0, Y1], M)
        torch.cuda.synchronize()
        out[tag] = [t.cpu().numpy().view(np.uint32) for t in (Y, Y0, Y1)]
    for x, y in zip(out["16"], out["64"]):
        np.testing.assert_array_equal(x, y)
    want = formula(S, c["sf"][:M], None, c["Bf"], "basic", "f32")
    np.testing.assert_array_equal(out["64"][1][:M], want)
    assert np.all(out["64"][1][M] == np.float32(SENT).view(np.uint32))
    assert [p.info()["device_bytes"] for p in (a64, b64)] == held
    for Wa, pa, Wb, pb in plans:
        pa.destroy(), pb.destroy(), Wa.free(), Wb.free()


def test_a_captured_call_replays_on_new_inputs(gpu, oracle, env):
    torch = gpu
    env()
    K, N, M = 1000, 300, 40
    c = case(oracle, K, N)
    W, plan = packed(c["Wd"], rows=1)
    on(plan, M)
    held = plan.info()["device_bytes"]
    side = torch.cuda.Stream()
    Qg = torch.zeros((M, K), dtype=torch.int8, device=DEV)
    Sg = torch.zeros(M, device=DEV)
    Yg = torch.empty((M, N), device=DEV)
    Bf = dev_f32(torch, c["Bf"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm_i8(Qg, Sg, Bf, Yg, M, N, "prelu_basic", A, torch.cuda.current_stream().cuda_stream)
    assert plan.info()["device_bytes"] == held
    for first in (0, 24):
        X = c["Xq"][first:first + M]
        Qg.copy_(dev_i8(torch, X))
        Sg.copy_(dev_f32(torch, c["sf"][first:first + M]))
        Yg.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = formula(int_sums(X, c["Wd"]), c["sf"][first:first + M], None, c["Bf"], "prelu_basic", "f32")
        np.testing.assert_array_equal(Yg.cpu().numpy().view(np.uint32), want, err_msg=f"replay from row {first}")
        assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()


# ---- 6. the setter ------------------------------------------------------------------------------------------------------

def test_the_setter(gpu, oracle, env):
    torch = gpu  # noqa: F841
    c = case(oracle, 65, 130)
    W, plan = packed(c["Wd"])
    assert plan.decode_rows == 16
    for rows in (16, 17, 40, 64, tcsc_amd.DECODE_ROWS_AUTO):
        plan.set_decode_rows(rows)
        assert plan.decode_rows == rows
    for M in (1, 16, 17, 32, 33, 64, 65):  # AUTO asks the rule, per call
        want = "decode" if M <= 16 or tcsc_amd.decode_rows_pays(M, 65, 130, torch.cuda.get_device_properties(0).multi_processor_count) else "mfma"
        assert plan.launch_info_i8(M)[0] == want, M
    plan.set_decode_rows(40)
    assert [plan.launch_info_i8(M)[0] for M in (16, 17, 40, 41, 64)] == ["decode", "decode", "decode", "mfma", "mfma"]
    for rows in (15, 65, 0, -2, 1 << 20):
        with pytest.raises(tcsc_amd.TcscError, match="tcsc_gpu_plan_set_decode_rows"):
            plan.set_decode_rows(rows)
        assert plan.decode_rows == 40
    for M in (0, 65):
        with pytest.raises(tcsc_amd.TcscError, match="tcsc_gpu_launch_info_decode"):
            plan.launch_info_decode(M)
    assert plan.launch_info_decode(16)[0] == 1 and plan.launch_info_decode(17)[0] == 2 and plan.launch_info_decode(33)[0] == 4
    plan.destroy()
    W.free()
    # a plan without the image
    env(TCSC_PATH="mfma")
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plain = tcsc_amd.Plan(W)
    plain.reserve(17)
    assert plain.enable_i8() and not plain.has_w2
    with pytest.raises(tcsc_amd.TcscError, match="2-bit image"):
        plain.set_decode_rows(64)
    assert plain.decode_rows == 16
    with pytest.raises(tcsc_amd.TcscError, match="tcsc_gpu_launch_info_decode"):
        plain.launch_info_decode(40)
    plain.destroy()
    W.free()


# ---- 7. the layer -------------------------------------------------------------------------------------------------------

def test_the_layer(gpu, oracle, env):
    torch = gpu
    env()
    from tcsc_amd.nn import PackedTernaryLinear

    K, N, M = 300, 130, 40
    c = case(oracle, K, N)
    x = dev_f32(torch, oracle.uniform((M, K), 27501))
    base = PackedTernaryLinear(c["Wd"], bias=c["Bf"], a=0.2, weight_scale=0.37)
    layer = PackedTernaryLinear(c["Wd"], bias=c["Bf"], a=0.2, weight_scale=0.37, decode_rows=64)
    assert base.plan.decode_rows == 16 and layer.plan.decode_rows == 64
    assert base.plan.launch_info_q8(M)[0] == "mfma" and layer.plan.launch_info_q8(M) == ("decode", 1, False)
    with torch.no_grad():
        y0, y1 = base(x), layer(x)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y1.cpu().numpy().view(np.uint32), y0.cpu().numpy().view(np.uint32))
    sd0, sd1 = base.state_dict(), layer.state_dict()
    assert list(sd0) == list(sd1) and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    empty = PackedTernaryLinear.empty(K, N, a=0.2, decode_rows=64)
    empty.load_state_dict(sd0)
    assert empty.plan.decode_rows == 64
    with torch.no_grad():
        y2 = empty(x)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y2.cpu().numpy().view(np.uint32), y0.cpu().numpy().view(np.uint32))
