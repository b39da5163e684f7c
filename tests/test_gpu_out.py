"""tcsc_gpu_sgemm_i8_out / tcsc_gpu_sgemm_q8_out: per-column weight scales and a bf16 Y in the epilogue of the int8
calls, on every kernel that finishes one: k_decode8q, k_decode8, k_gemm8w2, k_gemm8, k_reduce_i8.

The contract is an equality of bits, and there are two yardsticks, neither of them the code under test:
  (a) numpy: the quantizer restated in float32, the exact integer sums (every |S| asserted below 2^24), then in
      float32, one rounded operation per step,
          v = fl(fl(float(S) * s[m]) * c[j]);  v = fl(v + b[j]);  v = v < 0 ? a v : v
      and for a bf16 Y the rounding restated on the uint32 bits, (u + 0x7FFF + ((u >> 16) & 1)) >> 16;
  (b) the library's existing calls: with c NULL the bf16 Y is old_fp32_Y.to(torch.bfloat16); with c set, a zero
      bias and the identity the fp32 Y is old_Y * c (+ the zero bias, which turns a -0.0 product into +0.0) in
      torch fp32.
Y is compared as integer bits, and as the whole allocation: Y lives `off` elements into a sentinel-filled buffer of
max(16, M + 1) rows of pitch ldy, and the expected buffer is the sentinel everywhere but at rows < M, columns <
cols.  So the columns from cols to ldy, the rows from M on, the element before an offset base and -- for a bf16 Y --
the 2-byte element at column `cols` of an odd cols are all asserted unchanged by the one comparison.

Shapes: N around the 16-column tile, the 4-column store, an odd cols and the 128-wide GEMM tile; ldy = N, N + 1 and
the next multiple of 4 plus 4; the base also offset by one element (a bf16 Y 2-byte aligned only); K = 16, 257, 300
(unsplit) and 2049 (17 blocks of 128: K splits by default at M >= 17); M on every route: 1, 2, 4 fused under the
rule (and unfused under $TCSC_QFUSE=0), 5 and 16 k_decode8, 17 .. 130 k_gemm8w2 / k_gemm8 on both tile shapes with
ragged rows."""
import io

import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

A = 0.2
PRELU = pyoracle.PRELU_VARIANTS
VARIANTS = ("prelu_basic", "basic", "sparse_gemm", "prelu_onthego", "optimized", "prelu_separate")
KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")
NS = (1, 15, 16, 17, 33, 130, 260)
KS = (16, 257, 300, 2049)
DECODE_MS = (1, 2, 4, 5, 16)
GEMM_MS = (17, 40, 64, 65, 130)
ROWS = 130
XTYPES = ("f32", "bf16")
YTYPES = ("f32", "bf16")
SENT = 7.0  # 0x40E00000 as fp32, 0x40E0 as bf16


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


def np_bf16_bits(v):
    """Round to nearest even on the fp32 bits (finite inputs)."""
    v = np.ascontiguousarray(v, np.float32)
    assert np.isfinite(v).all()
    u = v.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def formula(S, s, c, b, variant, ytype, a=A):
    """The bits of Y (uint32 for an fp32 Y, uint16 for a bf16 one); s or c None: ones."""
    v = S.astype(np.float32)
    if s is not None:
        v = v * np.asarray(s, np.float32)[:, None]
    if c is not None:
        v = v * np.asarray(c, np.float32)[None, :]
    v = v + np.asarray(b, np.float32)[None, :]
    if variant in PRELU:
        v = np.where(v < 0, np.float32(a) * v, v)
    assert v.dtype == np.float32
    return np_bf16_bits(v) if ytype == "bf16" else np.ascontiguousarray(v).view(np.uint32)


def col_scales(N, seed):
    """1, 0.5, a non-power of two, a negative and 0.0 in the first five columns (as many as there are), a seeded mix
    of such values after them."""
    rng = np.random.default_rng(seed)
    pool = np.array([1.0, 0.5, 0.0123, -1.75, 0.0, 3.0, 0.3, -0.0625], np.float32)
    c = pool[rng.integers(0, pool.size, N)]
    c[:min(N, 5)] = pool[:min(N, 5)]
    return c.astype(np.float32)


_cases = {}


def case(torch, o, K, N, density=0.67):
    """W, ROWS rows of X in both types (the bf16 rows as their widened values) with the numpy quantization and exact
    sums of each, a float bias and the column scales -- computed once per shape and left unchanged.  A test of M
    rows uses the first M."""
    key = (K, N, density)
    if key not in _cases:
        seed = 21000 + 3 * K + 5 * N
        rng = np.random.default_rng(seed + 1)
        Wd = o.ternary((K, N), density, seed)
        X = (rng.standard_normal((ROWS, K)) * rng.choice([1e-3, 1.0, 37.0], (ROWS, 1))).astype(np.float32)
        X[2 % ROWS] = 0.0  # a row of zeros: scale 0
        Xb = torch.from_numpy(X).to(torch.bfloat16).to(torch.float32).numpy()
        c = dict(Wd=Wd, Bf=o.uniform((N,), seed + 3), Cs=col_scales(N, seed + 4), X={"f32": X, "bf16": Xb}, q={}, s={},
                 S={})
        for xt in XTYPES:
            c["q"][xt], c["s"][xt] = np_quantize(c["X"][xt])
            c["S"][xt] = int_sums(c["q"][xt], Wd)
        _cases[key] = c
    return _cases[key]


# ---- device buffers ---------------------------------------------------------------------------------------------------

DEV = "cuda:0"


def dev_f32(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def dev_x(torch, x, xt):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    return t if xt == "f32" else t.to(torch.bfloat16)


def ldys(N):
    return (N, N + 1, (N + 3) // 4 * 4 + 4)


def layouts(N):
    """(ldy, off) of a Y: the three pitches at an aligned base, and N and the round pitch at a base one element in."""
    a, b, r = ldys(N)
    return ((a, 0), (b, 0), (r, 0), (a, 1), (r, 1))


class YBuf:
    """A sentinel-filled allocation with Y at element `off`: max(16, M + 1) rows of pitch ldy."""

    def __init__(self, torch, M, N, ldy, off, ytype):
        self.torch, self.M, self.N, self.ldy, self.off, self.ytype = torch, M, N, ldy, off, ytype
        self.rows = max(16, M + 1)
        dt = torch.float32 if ytype == "f32" else torch.bfloat16
        self.buf = torch.full((off + self.rows * ldy + 8,), SENT, dtype=dt, device=DEV)
        self.Y = self.buf[off:]
        assert self.buf.data_ptr() % 16 == 0 and self.Y.data_ptr() == self.buf.data_ptr() + off * self.buf.element_size()

    def bits(self):
        """The whole allocation as integers."""
        self.torch.cuda.synchronize()
        if self.ytype == "f32":
            return self.buf.cpu().numpy().view(np.uint32)
        return self.buf.view(self.torch.int16).cpu().numpy().view(np.uint16)

    def expected(self, ybits):
        """The allocation with ybits (M x N) in place and the sentinel everywhere else."""
        sent = np.float32(SENT).view(np.uint32)
        want = np.full(self.buf.numel(), sent if self.ytype == "f32" else sent >> 16, ybits.dtype)
        idx = self.off + np.arange(self.M)[:, None] * self.ldy + np.arange(self.N)[None, :]
        want[idx] = ybits
        return want

    def check(self, ybits, what):
        got, want = self.bits(), self.expected(ybits)
        bad = np.flatnonzero(got != want)
        if bad.size:
            e = int(bad[0]) - self.off
            raise AssertionError(f"{what}: {bad.size} elements differ, the first at row {e // self.ldy} column "
                                 f"{e % self.ldy} (element {e} of Y, M={self.M} N={self.N} ldy={self.ldy} off={self.off}): "
                                 f"got {int(got[bad[0]]):#x}, expected {int(want[bad[0]]):#x}")

    def untouched(self):
        sent = int(np.float32(SENT).view(np.uint32))
        return bool(np.all(self.bits() == (sent if self.ytype == "f32" else sent >> 16)))

    def values(self):
        """Y[:M, :N] as bits."""
        idx = self.off + np.arange(self.M)[:, None] * self.ldy + np.arange(self.N)[None, :]
        return self.bits()[idx]


def run_q8(torch, plan, c, xt, M, N, ldy, off, ytype, cs, variant, B=None, a=A):
    """One sgemm_q8 (tcsc_gpu_sgemm_q8_out) on the first M rows; returns the YBuf and the scales."""
    X = dev_x(torch, c["X"][xt][:M], xt)
    yb = YBuf(torch, M, N, ldy, off, ytype)
    Xq = torch.empty((M, X.shape[1]), dtype=torch.int8, device=DEV)
    S = torch.full((M + 1,), 5.0, device=DEV)
    Bd = dev_f32(torch, c["Bf"] if B is None else B)
    Cd = None if cs is None else dev_f32(torch, cs)
    plan.sgemm_q8(X, Xq, S, Bd, yb.Y, M, ldy, variant, a, col_scale=Cd)
    torch.cuda.synchronize()
    S = S.cpu().numpy()
    assert S[M] == 5.0
    np.testing.assert_array_equal(S[:M].view(np.uint32), c["s"][xt][:M].view(np.uint32), err_msg="scales")
    return yb


def run_i8(torch, plan, q, s, M, N, ldy, off, ytype, cs, variant, B, a=A):
    """One sgemm_i8 (tcsc_gpu_sgemm_i8_out) on int8 rows q with row scales s (None: NULL)."""
    Xq = torch.from_numpy(np.ascontiguousarray(q[:M])).to(DEV)
    yb = YBuf(torch, M, N, ldy, off, ytype)
    Sd = None if s is None else dev_f32(torch, s[:M])
    Cd = None if cs is None else dev_f32(torch, cs)
    plan.sgemm_i8(Xq, Sd, dev_f32(torch, B), yb.Y, M, ldy, variant, a, col_scale=Cd)
    return yb


def sweep(torch, plan, c, N, Ms, what, start=0):
    """Every M, Y type and layout against yardstick (a); the column scales (NULL / set), the variant, the X type and
    the entry point (q8 on either X type, i8 with NULL and with real row scales) rotate so that each M and Y type
    meets both column-scale settings and several variants."""
    n = start
    for M in Ms:
        for ytype in YTYPES:
            for ldy, off in layouts(N):
                cs = c["Cs"] if n % 2 == 0 else None
                variant = VARIANTS[(n // 2) % len(VARIANTS)]
                kind = ("q8f", "q8b", "i8s", "i8n")[(n // 3) % 4]
                tag = f"{what} M={M} {ytype} ldy={ldy} off={off} cs={'set' if cs is not None else 'NULL'} {variant} {kind}"
                if kind in ("q8f", "q8b"):
                    xt = "f32" if kind == "q8f" else "bf16"
                    yb = run_q8(torch, plan, c, xt, M, N, ldy, off, ytype, cs, variant)
                    yb.check(formula(c["S"][xt][:M], c["s"][xt][:M], cs, c["Bf"], variant, ytype), tag)
                else:
                    s = c["s"]["f32"] if kind == "i8s" else None
                    yb = run_i8(torch, plan, c["q"]["f32"], s, M, N, ldy, off, ytype, cs, variant, c["Bf"])
                    yb.check(formula(c["S"]["f32"][:M], None if s is None else s[:M], cs, c["Bf"], variant, ytype), tag)
                n += 1
    return n


def packed_plan(Wd, rows=ROWS):
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan.packed(W)
    plan.reserve(rows)
    return W, plan


def ordinary_plan(env, Wd, rows=ROWS, **knobs):
    """An ordinary plan with the int8 and the 2-bit image (made under TCSC_PATH=mfma so that a small W gets them).
    A plan of fewer than 33 columns may come without the MFMA images: its merged CSC copy pads every 64-column
    group to the longest column, and the library drops a copy that is mostly padding (build_csc, tcsc_api.cpp) and the
    MFMA path with it.  Such a plan has no k_gemm8 to test and (W, None) is returned; from 33 columns on the images are
    asserted."""
    env(TCSC_PATH="mfma", **knobs)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan(W)
    plan.reserve(rows)
    if not plan.enable_i8():
        assert W.cols < 33, "an ordinary plan of 33 columns or more has the int8 image under TCSC_PATH=mfma"
        plan.destroy()
        return W, None
    assert plan.enable_w2()
    return W, plan


# ---- 1. the decode kernels ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_decode_routes(gpu, oracle, env, K, N):
    """M <= 16 on a packed plan: k_decode8q where the rule fuses (M = 1, 2, 4 at these sizes), k_decode8 at 5 and 16
    and, under $TCSC_QFUSE=0, at 1, 2, 4 too."""
    torch = gpu
    c = case(torch, oracle, K, N)
    env()
    W, plan = packed_plan(c["Wd"])
    for M in DECODE_MS:
        for xt in XTYPES:
            assert plan.launch_info_q8(M, xt) == ("decode", 1, M <= 4), (M, xt)
        assert plan.launch_info_i8(M) == ("decode", 1)
    n = sweep(torch, plan, c, N, DECODE_MS, "decode")
    env(TCSC_QFUSE="0")
    for M in (1, 2, 4):
        assert plan.launch_info_q8(M, "bf16") == ("decode", 1, False)
    sweep(torch, plan, c, N, (1, 2, 4), "decode QFUSE=0", start=n + 1)
    plan.destroy()
    W.free()


# ---- 2. the GEMM kernels -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_gemm_routes(gpu, oracle, env, K, N):
    """M >= 17: k_gemm8w2 on a packed plan, k_gemm8 on an ordinary one and k_gemm8w2 there under $TCSC_W2GEMM=1; the
    64 x 256 tiles up to 64 rows, the 128 x 128 ones above; K = 2049 splits by the default rule (k_reduce_i8)."""
    torch = gpu
    c = case(torch, oracle, K, N)
    env()
    W, plan = packed_plan(c["Wd"])
    slices = {M: plan.launch_info_i8(M)[1] for M in GEMM_MS}
    for M in GEMM_MS:
        assert plan.launch_info_i8(M)[0] == "mfma" and plan.launch_info_q8(M, "f32") == ("mfma", slices[M], False)
        assert (slices[M] > 1) == (K == 2049), (M, slices[M])
    n = sweep(torch, plan, c, N, GEMM_MS, "k_gemm8w2")
    plan.destroy()
    W.free()
    W, plan = ordinary_plan(env, c["Wd"])
    if plan is None:
        W.free()
        return
    assert plan.has_i8 and plan.has_w2 and not plan.is_packed
    for knob in (None, "1"):
        env(TCSC_PATH="mfma", TCSC_W2GEMM=knob)
        for M in GEMM_MS:
            assert plan.launch_info_i8(M) == ("mfma", slices[M]), M
        n = sweep(torch, plan, c, N, GEMM_MS, f"ordinary plan W2GEMM={knob}", start=n + 1)
    plan.destroy()
    W.free()


@pytest.mark.parametrize("N,wgs,vec", [(260, 4, True), (33, 2, False)])
def test_a_pinned_split_runs_the_reduce(gpu, oracle, env, N, wgs, vec):
    """$TCSC_MFMA_WGS pins two K slices at M = 40, K = 2049: k_reduce_i8 in its 4-column form at N = 260 (where ldy %
    4 == 0 and Y is aligned to four elements) and in its scalar form at N = 33; the bits of the unsplit call."""
    torch = gpu
    K, M = 2049, 40
    c = case(torch, oracle, K, N)
    env(TCSC_MFMA_WGS="0")
    W, plan = packed_plan(c["Wd"])
    Wo, other = ordinary_plan(env, c["Wd"], TCSC_MFMA_WGS="0")
    for p in (plan, other):
        assert p.launch_info_i8(M) == ("mfma", 1)
    unsplit = {}
    for ytype in YTYPES:
        for ldy, off in layouts(N):
            yb = run_q8(torch, plan, c, "bf16", M, N, ldy, off, ytype, c["Cs"], "prelu_basic")
            yb.check(formula(c["S"]["bf16"][:M], c["s"]["bf16"][:M], c["Cs"], c["Bf"], "prelu_basic", ytype), "unsplit")
            unsplit[ytype, ldy, off] = yb.values()
    for p, knobs in ((plan, {}), (other, dict(TCSC_PATH="mfma")), (other, dict(TCSC_PATH="mfma", TCSC_W2GEMM="1"))):
        env(TCSC_MFMA_WGS=wgs, **knobs)
        assert p.launch_info_i8(M) == ("mfma", 2)
        for ytype in YTYPES:
            for ldy, off in layouts(N):
                yb = run_q8(torch, p, c, "bf16", M, N, ldy, off, ytype, c["Cs"], "prelu_basic")
                yb.check(unsplit[ytype, ldy, off], f"split, {knobs} {ytype} ldy={ldy} off={off} (vec form: "
                                                   f"{vec and ldy % 4 == 0 and off == 0})")
    plan.destroy()
    other.destroy()
    W.free()
    Wo.free()


# ---- 3. yardstick (b): the existing calls --------------------------------------------------------------------------------

def old_q8(torch, plan, c, xt, M, N, variant, B):
    """tcsc_gpu_sgemm_q8 itself (the entry point as it was): an fp32 Y, as a tensor."""
    X = dev_x(torch, c["X"][xt][:M], xt)
    Y = torch.empty((M, N), device=DEV)
    Xq = torch.empty((M, X.shape[1]), dtype=torch.int8, device=DEV)
    S = torch.empty(M, device=DEV)
    Bd = dev_f32(torch, B)
    import ctypes as C
    rc = tcsc_amd.lib().tcsc_gpu_sgemm_q8(plan.handle, C.c_void_p(X.data_ptr()), tcsc_amd.XTYPE_ID[xt],
                                          C.c_void_p(Xq.data_ptr()), C.c_void_p(S.data_ptr()), C.c_void_p(Bd.data_ptr()),
                                          C.c_void_p(Y.data_ptr()), M, N, tcsc_amd.VARIANT_ID[variant], A, None)
    assert rc == 0, tcsc_amd.last_error()
    torch.cuda.synchronize()
    return Y


@pytest.mark.parametrize("K,N", [(300, 33), (2049, 260), (257, 130)])
def test_against_the_existing_calls(gpu, oracle, env, K, N):
    torch = gpu
    c = case(torch, oracle, K, N)
    env()
    W, plan = packed_plan(c["Wd"])
    Wo, other = ordinary_plan(env, c["Wd"])
    zero = np.zeros(N, np.float32)
    for p, Ms in ((plan, DECODE_MS + GEMM_MS), (other, GEMM_MS)):
        for i, M in enumerate(Ms):
            xt = XTYPES[i % 2]
            variant = "prelu_basic" if i % 3 else "basic"
            old = old_q8(torch, p, c, xt, M, N, variant, c["Bf"])
            # c NULL: the fp32 Y is the old one, the bf16 Y its conversion
            yb = run_q8(torch, p, c, xt, M, N, N + 1, 1, "f32", None, variant)
            yb.check(old.cpu().numpy().view(np.uint32), f"M={M} fp32, no column scale")
            yb = run_q8(torch, p, c, xt, M, N, N + 1, 1, "bf16", None, variant)
            yb.check(old.to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16), f"M={M} bf16 of the old Y")
            # c set, a zero bias, the identity: old_Y * c in torch fp32 -- and then the zero bias added, as the
            # epilogue adds it after the scale: where a product is -0.0 (c = 0.0 under a negative sum, a negative c
            # under a zero row) fl(-0.0 + 0.0) is +0.0, and old_Y * c alone would keep the sign
            old0 = old_q8(torch, p, c, xt, M, N, "basic", zero)
            want = old0 * dev_f32(torch, c["Cs"])[None, :] + dev_f32(torch, zero)[None, :]
            yb = run_q8(torch, p, c, xt, M, N, N, 0, "f32", c["Cs"], "basic", B=zero)
            yb.check(want.cpu().numpy().view(np.uint32), f"M={M} old_Y * c")
    plan.destroy()
    other.destroy()
    W.free()
    Wo.free()


# ---- 4. the same bits on every route ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,N", [(300, 33), (2049, 260)])
def test_equal_bits_across_routes(gpu, oracle, env, K, N):
    """The same q and s through sgemm_i8: k_decode8 at M = 16 against rows 0 .. 15 of an M = 17 call (k_gemm8w2),
    a packed against an ordinary plan (k_gemm8), a split against an unsplit K."""
    torch = gpu
    c = case(torch, oracle, K, N)
    q, s = c["q"]["bf16"], c["s"]["bf16"]
    env()
    W, plan = packed_plan(c["Wd"])
    assert plan.launch_info_i8(16) == ("decode", 1) and plan.launch_info_i8(17)[0] == "mfma"
    Wo, other = ordinary_plan(env, c["Wd"])
    for ytype in YTYPES:
        for variant in ("prelu_basic", "sparse_gemm"):
            env()
            y16 = run_i8(torch, plan, q, s, 16, N, N + 1, 1, ytype, c["Cs"], variant, c["Bf"]).values()
            y17 = run_i8(torch, plan, q, s, 17, N, N + 1, 1, ytype, c["Cs"], variant, c["Bf"]).values()
            np.testing.assert_array_equal(y16, y17[:16], err_msg=f"decode against k_gemm8w2 {ytype} {variant}")
            np.testing.assert_array_equal(y17, formula(c["S"]["bf16"][:17], s[:17], c["Cs"], c["Bf"], variant, ytype))
            for M in (40, 130):
                env()
                yp = run_i8(torch, plan, q, s, M, N, N, 0, ytype, c["Cs"], variant, c["Bf"]).values()
                env(TCSC_PATH="mfma")
                assert other.launch_info_i8(M) == plan.launch_info_i8(M)
                yo = run_i8(torch, other, q, s, M, N, N, 0, ytype, c["Cs"], variant, c["Bf"]).values()
                np.testing.assert_array_equal(yp, yo, err_msg=f"packed against ordinary M={M} {ytype} {variant}")
                env(TCSC_MFMA_WGS="0")
                assert plan.launch_info_i8(M) == ("mfma", 1)
                yu = run_i8(torch, plan, q, s, M, N, N, 0, ytype, c["Cs"], variant, c["Bf"]).values()
                np.testing.assert_array_equal(yp, yu, err_msg=f"default split against unsplit M={M} {ytype} {variant}")
    env()
    assert (plan.launch_info_i8(40)[1] > 1) == (K == 2049)
    plan.destroy()
    other.destroy()
    W.free()
    Wo.free()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------

def test_the_gather_route_takes_the_plain_call_only(gpu, oracle, env):
    """An ordinary plan of a 2 %-dense W routes to the gather: (NULL, fp32) is sgemm_i8, anything else TCSC_E_ARG
    naming the call and the path, and Y is not touched."""
    import ctypes as C

    torch = gpu
    K, N, M = 300, 33, 40
    c = case(torch, oracle, K, N, density=0.02)
    env()
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan(W)
    plan.reserve(M)
    assert plan.launch_info_i8(M)[0] == "gather" and plan.launch_info_q8(M, "f32")[0] == "gather"
    q, s = c["q"]["f32"], c["s"]["f32"]
    Xq, Sd, Bd = torch.from_numpy(q[:M].copy()).to(DEV), dev_f32(torch, s[:M]), dev_f32(torch, c["Bf"])
    old = torch.empty((M, N), device=DEV)
    rc = tcsc_amd.lib().tcsc_gpu_sgemm_i8(plan.handle, C.c_void_p(Xq.data_ptr()), C.c_void_p(Sd.data_ptr()),
                                          C.c_void_p(Bd.data_ptr()), C.c_void_p(old.data_ptr()), M, N,
                                          tcsc_amd.VARIANT_ID["prelu_basic"], A, None)
    assert rc == 0, tcsc_amd.last_error()
    torch.cuda.synchronize()
    yb = run_i8(torch, plan, q, s, M, N, N + 1, 1, "f32", None, "prelu_basic", c["Bf"])
    yb.check(old.cpu().numpy().view(np.uint32), "(NULL, fp32) on the gather")
    yb = run_q8(torch, plan, c, "f32", M, N, N + 1, 1, "f32", None, "prelu_basic")
    yb.check(old.cpu().numpy().view(np.uint32), "q8 (NULL, fp32) on the gather")
    for ytype, cs in (("bf16", None), ("f32", c["Cs"]), ("bf16", c["Cs"])):
        with pytest.raises(tcsc_amd.TcscError, match=r"tcsc_gpu_sgemm_i8_out.*gather"):
            run_i8(torch, plan, q, s, M, N, N, 0, ytype, cs, "prelu_basic", c["Bf"])
        with pytest.raises(tcsc_amd.TcscError, match=r"tcsc_gpu_sgemm_q8_out.*gather"):
            run_q8(torch, plan, c, "f32", M, N, N, 0, ytype, cs, "prelu_basic")
        yb = YBuf(torch, M, N, N, 0, ytype)
        Cd = None if cs is None else dev_f32(torch, cs)
        with pytest.raises(tcsc_amd.TcscError, match="gather"):
            plan.sgemm_i8(Xq, Sd, Bd, yb.Y, M, N, "prelu_basic", A, col_scale=Cd)
        assert yb.untouched(), "a refused call wrote Y"
    plan.destroy()
    W.free()


def test_a_live_plan_refuses_a_bad_ytype_and_a_null_y(gpu, oracle, env):
    torch = gpu
    K, N, M = 300, 33, 4
    c = case(torch, oracle, K, N)
    env()
    W, plan = packed_plan(c["Wd"])
    X = dev_x(torch, c["X"]["f32"][:M], "f32")
    Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
    S, Bd, Y = torch.empty(M, device=DEV), dev_f32(torch, c["Bf"]), torch.empty((M, N), device=DEV)
    for yt in (2, -1):
        with pytest.raises(tcsc_amd.TcscError, match=r"tcsc_gpu_sgemm_q8_out.*ytype"):
            plan.sgemm_q8(X, Xq, S, Bd, Y, M, N, ytype=yt)
        with pytest.raises(tcsc_amd.TcscError, match=r"tcsc_gpu_sgemm_i8_out.*ytype"):
            plan.sgemm_i8(Xq, S, Bd, Y, M, N, ytype=yt)
    with pytest.raises(tcsc_amd.TcscError, match=r"tcsc_gpu_sgemm_q8_out.*NULL"):
        plan.sgemm_q8(X, Xq, S, Bd, None, M, N, ytype="bf16")
    with pytest.raises(tcsc_amd.TcscError, match=r"tcsc_gpu_sgemm_i8_out.*NULL"):
        plan.sgemm_i8(Xq, S, Bd, None, M, N)
    with pytest.raises(tcsc_amd.TcscError, match=r"tcsc_gpu_sgemm_i8_out.*NULL"):
        plan.sgemm_i8(Xq, S, None, Y, M, N)
    plan.destroy()
    W.free()


# ---- 6. capture ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 40])
def test_a_captured_call_replays_on_new_inputs(gpu, oracle, env, M):
    """After reserve(64): sgemm_q8 with column scales and a bf16 Y captured on one stream, replayed on a new X: the
    bits of the eager call, and the plan holds what it held."""
    torch = gpu
    K, N = 300, 33
    c = case(torch, oracle, K, N)
    env()
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan.packed(W)
    plan.reserve(64)
    held = plan.info()["device_bytes"]
    Xg = torch.zeros((M, K), dtype=torch.bfloat16, device=DEV)
    Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
    Sg, Yg = torch.zeros(M, device=DEV), torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    Bd, Cd = dev_f32(torch, c["Bf"]), dev_f32(torch, c["Cs"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm_q8(Xg, Xq, Sg, Bd, Yg, M, N, "prelu_basic", A, torch.cuda.current_stream().cuda_stream, col_scale=Cd)
    for r0 in (0, 50):
        Xg.copy_(dev_x(torch, c["X"]["bf16"][r0:r0 + M], "bf16"))
        Yg.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = Yg.view(torch.int16).cpu().numpy().view(np.uint16)
        Ye = torch.full((M, N), SENT, dtype=torch.bfloat16, device=DEV)
        plan.sgemm_q8(Xg, Xq, Sg, Bd, Ye, M, N, "prelu_basic", A, col_scale=Cd)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got, Ye.view(torch.int16).cpu().numpy().view(np.uint16), err_msg=f"rows {r0}..")
        rows = slice(r0, r0 + M)
        np.testing.assert_array_equal(got, formula(c["S"]["bf16"][rows], c["s"]["bf16"][rows], c["Cs"], c["Bf"],
                                                   "prelu_basic", "bf16"))
    assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()


# ---- 7. the layer ----------------------------------------------------------------------------------------------------------

def test_the_layer_scales_and_returns_bf16(gpu, oracle, env):
    torch = gpu
    from tcsc_amd.nn import PackedTernaryLinear

    K, N = 300, 33
    c = case(torch, oracle, K, N)
    env()
    for ws, cs in ((c["Cs"], c["Cs"]), (0.3, np.full(N, 0.3, np.float32))):
        layer = PackedTernaryLinear(c["Wd"], c["Bf"], a=A, weight_scale=ws, out_dtype=torch.bfloat16)
        assert layer.weight_scale.shape == (N,) and layer.weight_scale.dtype == torch.float32
        for M in (3, 40):
            for xt in XTYPES:
                y = layer(dev_x(torch, c["X"][xt][:M], xt))
                assert y.dtype == torch.bfloat16 and y.shape == (M, N)
                np.testing.assert_array_equal(
                    y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16),
                    formula(c["S"][xt][:M], c["s"][xt][:M], cs, c["Bf"], "prelu_basic", "bf16"), err_msg=f"M={M} {xt}")
    # the state_dict carries weight_scale, through torch.save and back into an empty layer
    sd = layer.state_dict()
    assert set(sd) == {"bias", "w2", "weight_scale"} and sd["weight_scale"].numel() == N
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    loaded = PackedTernaryLinear.empty(K, N, a=A, out_dtype=torch.bfloat16)
    assert loaded.weight_scale is None
    loaded.load_state_dict(torch.load(f))
    assert torch.equal(loaded.weight_scale, layer.weight_scale) and loaded.weight_scale.device.type == "cuda"
    x = dev_x(torch, c["X"]["bf16"][:40], "bf16")
    assert torch.equal(loaded(x).view(torch.int16), layer(x).view(torch.int16))
    with pytest.raises(tcsc_amd.TcscError, match="weight_scale"):
        bad = dict(sd)
        bad["weight_scale"] = torch.zeros(N + 1)
        PackedTernaryLinear.empty(K, N).load_state_dict(bad)
    # a layer without a scale keeps exactly the two keys, returns fp32 by default, and loads into a scaled layer as unscaled
    plain = PackedTernaryLinear(c["Wd"], c["Bf"], a=A)
    assert set(plain.state_dict()) == {"bias", "w2"} and plain.weight_scale is None
    y = plain(x)
    assert y.dtype == torch.float32
    np.testing.assert_array_equal(y.cpu().numpy().view(np.uint32),
                                  formula(c["S"]["bf16"][:40], c["s"]["bf16"][:40], None, c["Bf"], "prelu_basic", "f32"))
    loaded.load_state_dict(plain.state_dict())
    assert loaded.weight_scale is None
    with pytest.raises(tcsc_amd.TcscError, match="out_dtype"):
        PackedTernaryLinear(c["Wd"], out_dtype=torch.float16)
    with pytest.raises(tcsc_amd.TcscError, match="weight_scale"):
        PackedTernaryLinear(c["Wd"], weight_scale=np.ones(N + 1, np.float32))


def test_from_float(gpu, env):
    torch = gpu
    from tcsc_amd.nn import PackedTernaryLinear

    env()
    K, N = 300, 33
    Wf = (np.random.default_rng(2107).standard_normal((K, N)) * 0.02).astype(np.float32)
    T, beta = tcsc_amd.ternarize_absmean(Wf)
    layer = PackedTernaryLinear.from_float(Wf, a=None, out_dtype=torch.bfloat16)
    ref = PackedTernaryLinear(T, weight_scale=float(beta), out_dtype=torch.bfloat16)
    assert torch.equal(layer.state_dict()["w2"], ref.state_dict()["w2"])  # the plan of T
    assert layer.nnz == int(np.count_nonzero(T))
    want = torch.full((N,), float(beta), dtype=torch.float32, device=DEV)
    assert torch.equal(layer.weight_scale, want) and layer.out_dtype == torch.bfloat16
    layer2 = PackedTernaryLinear.from_float(torch.from_numpy(Wf))
    assert torch.equal(layer2.state_dict()["w2"], ref.state_dict()["w2"]) and layer2.out_dtype == torch.float32
