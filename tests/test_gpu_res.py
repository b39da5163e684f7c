"""tcsc_gpu_sgemm_i8_res / tcsc_gpu_sgemm_q8_res: the residual add in the epilogue of the int8 calls,
Y = R + X W, on every kernel that finishes one: k_decode8q (with and without the norm), k_decode8, k_gemm8w2, k_gemm8
and k_reduce_i8, out of place and in place.

The contract is an equality of bits, and the yardsticks are those of tests/test_gpu_out.py, neither of them the code
under test:
  (a) numpy: the quantizer, the exact integer sums (every |S| asserted below 2^24) and formula() of that file for
      v, then y = fl(v + r) as one float32 add and, for a bf16 Y, the rounding restated on the uint32 bits;
  (b) the library's existing call: sgemm_i8 with the column scales into an fp32 Y0, then torch's Y0 + R.float() and
      .to(torch.bfloat16).
Y is compared as integer bits over its whole sentinel-filled allocation (YBuf of that file).  R lives in a
sentinel-filled allocation of its own, at a pitch and a base offset that rotate independently of Y's -- so the
four-column accesses fall back to single elements from R's side, from Y's side and from both -- and is asserted
unchanged after every out-of-place call.  In place, Y's allocation holds R at rows < M, columns < cols and the
sentinel elsewhere, and the result must be the out-of-place one.

R's values: a seeded normal mix of three magnitudes, +0, -0, +-1e30, and -v itself at a handful of positions of an
fp32 R (the sum is then +0).  Row 2 of X is zero, so v there is the bias, and the bias of this file has columns whose
value plus R = 0.5 is exactly half-way between two bf16 values (one tie rounds down to the even neighbour, one up) and
columns that cancel against R to +0; the test asserts that those sums are the ties they are meant to be."""
import numpy as np
import pytest

import norm_cases as nc
import tcsc_amd
from test_gpu_out import (DECODE_MS, DEV, GEMM_MS, KNOBS, KS, NS, SENT, XTYPES, YTYPES, YBuf, case, dev_f32, dev_x, formula,
                          int_sums, layouts, np_bf16_bits, np_quantize, ordinary_plan, packed_plan)

pytestmark = pytest.mark.gpu

KINDS = ("q8f", "q8b", "i8s", "i8n")  # fp32 / bf16 X through sgemm_q8; int8 X with and without row scales
TIE_DOWN, TIE_UP, CANCEL = np.float32(0.50390625), np.float32(0.51171875), np.float32(-1.75)
EPS = 1e-5


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    lib = tcsc_amd.lib()
    for name in ("tcsc_gpu_sgemm_i8_res", "tcsc_gpu_sgemm_q8_res"):  # without the feature every test fails here
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

def res_bias(c):
    """The shape's bias with the special columns: j % 5 == 0 and 1 the two ties, j % 5 == 2 the cancelling value."""
    b = np.array(c["Bf"], np.float32)
    for k, val in enumerate((TIE_DOWN, TIE_UP, CANCEL)):
        b[k::5] = val
    return b


def kind_inputs(c, kind, M):
    """(x type or None, q, s, S) of the first M rows for an input kind."""
    xt = {"q8f": "f32", "q8b": "bf16"}.get(kind, "f32")
    s = None if kind == "i8n" else c["s"][xt][:M]
    return xt, c["q"][xt][:M], s, c["S"][xt][:M]


def value(c, kind, M, cs, b):
    """v of yardstick (a) as float32: tcsc_gpu_sgemm_i8_out's fp32 value without PReLU."""
    _, _, s, S = kind_inputs(c, kind, M)
    return formula(S, s, cs, b, "basic", "f32").view(np.float32)


def to_bf16_f32(torch, a):
    """a rounded to bf16, as float32 values."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def r_values(torch, v, ytype, seed):
    """R for the values v (M x N float32), as float32 values representable in ytype."""
    rng = np.random.default_rng(seed)
    M, N = v.shape
    R = (rng.standard_normal((M, N)) * rng.choice([1e-3, 1.0, 50.0], (M, N))).astype(np.float32)
    pos = rng.permutation(M * N)
    flat = R.reshape(-1)
    special = np.array([0.0, -0.0, 1e30, -1e30], np.float32)
    flat[pos[:4]] = special[:min(4, pos.size)]
    if ytype == "f32":
        flat[pos[4:9]] = -v.reshape(-1)[pos[4:9]]  # the sum is +0
    else:
        R = to_bf16_f32(torch, R)
    if M > 2:  # the zero row of X: v is the bias
        R[2, 0::5] = 0.5
        R[2, 1::5] = 0.5
        R[2, 2::5] = 1.75
    return R


def r_bits(R, ytype):
    R = np.ascontiguousarray(R, np.float32)
    u = R.view(np.uint32)
    if ytype == "f32":
        return u.copy()
    assert not np.any(u & 0xFFFF), "a bf16 R holds bf16 values"
    return (u >> 16).astype(np.uint16)


def add(v, R, ytype):
    """y = fl(v + r): the bits of Y."""
    y = v.astype(np.float32) + R.astype(np.float32)
    assert y.dtype == np.float32
    return np_bf16_bits(y) if ytype == "bf16" else np.ascontiguousarray(y).view(np.uint32)


def assert_ties(v, R, M):
    """Row 2: columns 0 and 1 (mod 5) sum to a value half-way between two bf16 values, column 2 to +0."""
    if M <= 2:
        return
    y = (v[2] + R[2]).astype(np.float32).view(np.uint32)
    assert np.all(y[0::5] & 0xFFFF == 0x8000) and np.all(y[1::5] & 0xFFFF == 0x8000)
    assert np.all((y[0::5] >> 16) & 1 == 0) and np.all((y[1::5] >> 16) & 1 == 1)  # one rounds down, one up
    assert np.all(y[2::5] == 0)


# ---- device buffers ---------------------------------------------------------------------------------------------------

def fill(yb, bits):
    """A YBuf with `bits` (M x N) at rows < M, columns < cols and the sentinel elsewhere."""
    torch = yb.torch
    want = yb.expected(bits)
    if yb.ytype == "f32":
        yb.buf.view(torch.int32).copy_(torch.from_numpy(want.view(np.int32)).to(DEV))
    else:
        yb.buf.view(torch.int16).copy_(torch.from_numpy(want.view(np.int16)).to(DEV))
    return yb


def r_layout(N, n):
    """(ldr, offset) of R for the n-th call: test_gpu_out's layouts, rotating against Y's."""
    lay = layouts(N)
    return lay[(n // len(lay) + 2 * n + 1) % len(lay)]


def call(torch, plan, c, kind, M, yb, R, ldr, cs, b, norm=None):
    """One residual call on the first M rows into yb; R is a tensor (a YBuf's Y: in place it is yb.Y itself)."""
    xt, q, s, _ = kind_inputs(c, kind, M)
    Bd = dev_f32(torch, b)
    Cd = None if cs is None else dev_f32(torch, cs)
    if kind in ("q8f", "q8b"):
        X = dev_x(torch, c["X"][xt][:M], xt)
        Xq = torch.empty((M, X.shape[1]), dtype=torch.int8, device=DEV)
        S = torch.full((M + 1,), 5.0, device=DEV)
        if norm is None:
            plan.sgemm_q8(X, Xq, S, Bd, yb.Y, M, yb.ldy, "basic", 0.0, col_scale=Cd, residual=R, ldr=ldr)
        else:
            plan.sgemm_q8_norm(X, Xq, S, Bd, yb.Y, M, yb.ldy, norm[0], norm[1], "basic", 0.0, col_scale=Cd, residual=R,
                               ldr=ldr)
        torch.cuda.synchronize()
        S = S.cpu().numpy()
        assert S[M] == 5.0
        return S[:M]
    Xq = torch.from_numpy(np.ascontiguousarray(q)).to(DEV)
    Sd = None if s is None else dev_f32(torch, s)
    plan.sgemm_i8(Xq, Sd, Bd, yb.Y, M, yb.ldy, "basic", 0.0, col_scale=Cd, residual=R, ldr=ldr)
    return None


def both_ways(torch, plan, c, kind, M, N, ldy, off, ldr, roff, ytype, cs, b, tag):
    """Out of place against yardstick (a) with R unchanged, then in place: the same bits.  Returns Y[:M, :N]."""
    v = value(c, kind, M, cs, b)
    R = r_values(torch, v, ytype, 7 * M + N + ldr)
    assert_ties(v, R, M)
    want = add(v, R, ytype)
    rb = fill(YBuf(torch, M, N, ldr, roff, ytype), r_bits(R, ytype))
    yb = YBuf(torch, M, N, ldy, off, ytype)
    s = call(torch, plan, c, kind, M, yb, rb.Y, ldr, cs, b)
    if s is not None:
        xt = kind_inputs(c, kind, M)[0]
        np.testing.assert_array_equal(s.view(np.uint32), c["s"][xt][:M].view(np.uint32), err_msg=f"{tag}: scales")
    yb.check(want, tag)
    rb.check(r_bits(R, ytype), f"{tag}: R was written")
    ib = fill(YBuf(torch, M, N, ldy, off, ytype), r_bits(R, ytype))
    call(torch, plan, c, kind, M, ib, ib.Y, ldy, cs, b)
    ib.check(want, f"{tag}: in place")
    return yb.values()


def sweep(torch, plan, c, N, Ms, what, start=0):
    """Every M, Y type and Y layout; R's layout, the column scales and the input kind rotate."""
    n = start
    b = res_bias(c)
    for M in Ms:
        for ytype in YTYPES:
            for ldy, off in layouts(N):
                ldr, roff = r_layout(N, n)
                cs = c["Cs"] if n % 2 == 0 else None
                kind = KINDS[(n // 3) % 4]
                tag = (f"{what} M={M} {ytype} ldy={ldy} off={off} ldr={ldr} roff={roff} "
                       f"cs={'set' if cs is not None else 'NULL'} {kind}")
                both_ways(torch, plan, c, kind, M, N, ldy, off, ldr, roff, ytype, cs, b, tag)
                n += 1
    return n


def test_the_r_layouts_meet_every_alignment_pair(gpu):
    """Over a sweep's calls, an aligned Y meets an R one element in and the reverse, and both vector-ready pitches
    meet: the fallback of the four-column access is reached from either side."""
    for N in NS:
        seen = set()
        for n, (ldy, off) in enumerate(layouts(N) * 4):
            ldr, roff = r_layout(N, n)
            seen.add((ldy % 4 == 0 and off == 0, ldr % 4 == 0 and roff == 0))
            assert ldr in (N, N + 1, (N + 3) // 4 * 4 + 4) and roff in (0, 1)
        assert {(True, False), (False, True), (True, True)} <= seen, (N, seen)


# ---- 1. the decode kernels ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_decode_routes(gpu, oracle, env, K, N):
    """M <= 16 on a packed plan: k_decode8q where the rule fuses (M = 1, 2, 4), k_decode8 at 5 and 16 and, under
    $TCSC_QFUSE=0, at 1, 2, 4 too."""
    torch = gpu
    c = case(torch, oracle, K, N)
    env()
    W, plan = packed_plan(c["Wd"])
    for M in DECODE_MS:
        assert plan.launch_info_q8(M, "bf16") == ("decode", 1, M <= 4) and plan.launch_info_i8(M) == ("decode", 1)
    n = sweep(torch, plan, c, N, DECODE_MS, "decode")
    env(TCSC_QFUSE="0")
    assert plan.launch_info_q8(4, "bf16") == ("decode", 1, False)
    sweep(torch, plan, c, N, (1, 2, 4), "decode QFUSE=0", start=n + 1)
    plan.destroy()
    W.free()


@pytest.mark.parametrize("M,N,T", [(8, 8256, 2), (16, 16512, 4)])
def test_two_and_four_tiles_per_workgroup(gpu, oracle, env, M, N, T):
    """The instantiations small shapes never reach on 256 CUs: one grid of 258 workgroups at T = 2 and at T = 4, the
    quantizer outside and (under $TCSC_QFUSE=1) inside the launch."""
    torch = gpu
    K = 16
    assert ((N + 15) // 16 + T - 1) // T == 258
    rng = np.random.default_rng(2600 + T)
    Wd = oracle.ternary((K, N), 0.67, 2600 + T)
    X = rng.standard_normal((M, K)).astype(np.float32)
    X[2] = 0.0
    q, s = np_quantize(X)
    c = dict(Wd=Wd, Bf=oracle.uniform((N,), 2610 + T), Cs=None, X={"f32": X}, q={"f32": q}, s={"f32": s},
             S={"f32": int_sums(q, Wd)})
    b = res_bias(c)
    env()
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan.packed(W)
    for knob, fused in ((None, False), ("1", True)):
        env(TCSC_QFUSE=knob)
        assert plan.launch_info_q8(M, "f32") == ("decode", 1, fused)
        for i, ytype in enumerate(YTYPES):
            both_ways(torch, plan, c, "q8f", M, N, N + 4 * i, i, N + 1 - i, 1 - i, ytype, None, b,
                      f"T={T} QFUSE={knob} {ytype}")
    plan.destroy()
    W.free()


# ---- 2. the GEMM kernels -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_gemm_routes(gpu, oracle, env, K, N):
    """M >= 17: k_gemm8w2 on a packed plan and k_gemm8 on an ordinary one with the int8 image; the 64 x 256 tiles up to
    64 rows, the 128 x 128 ones above.  K = 2049 splits by the default rule (k_reduce_i8, with and without VEC as the
    layouts rotate) and runs unsplit under $TCSC_MFMA_WGS=0."""
    torch = gpu
    c = case(torch, oracle, K, N)
    env()
    W, plan = packed_plan(c["Wd"])
    Wo, other = ordinary_plan(env, c["Wd"])
    n = 0
    for p, knobs, what in ((plan, {}, "k_gemm8w2"), (other, dict(TCSC_PATH="mfma"), "k_gemm8")):
        if p is None:
            continue
        env(**knobs)
        for M in GEMM_MS:
            path, slices = p.launch_info_i8(M)
            assert path == "mfma" and (slices > 1) == (K == 2049), (what, M, slices)
        n = sweep(torch, p, c, N, GEMM_MS, what, start=n + 1)
        if K == 2049:
            env(TCSC_MFMA_WGS="0", **knobs)
            assert p.launch_info_i8(40) == ("mfma", 1)
            n = sweep(torch, p, c, N, (17, 65), f"{what} unsplit", start=n + 1)
    plan.destroy()
    W.free()
    if other is not None:
        other.destroy()
    Wo.free()


@pytest.mark.parametrize("N,wgs", [(260, 4), (33, 2)])
def test_a_pinned_split_runs_the_reduce(gpu, oracle, env, N, wgs):
    """$TCSC_MFMA_WGS pins two K slices at M = 40, K = 2049: k_reduce_i8 with the residual, in its 4-column form where
    Y and R are both vector-ready and in its scalar form elsewhere; the bits of the unsplit call."""
    torch = gpu
    K, M = 2049, 40
    c = case(torch, oracle, K, N)
    b = res_bias(c)
    env(TCSC_MFMA_WGS=wgs)
    W, plan = packed_plan(c["Wd"])
    assert plan.launch_info_i8(M) == ("mfma", 2)
    for ytype in YTYPES:
        for (ldy, off), (ldr, roff) in zip(layouts(N), layouts(N)[3:] + layouts(N)[:3]):
            for lr, ro in ((ldr, roff), (ldy, off)):
                both_ways(torch, plan, c, "q8b", M, N, ldy, off, lr, ro, ytype, c["Cs"], b,
                          f"two slices {ytype} ldy={ldy} off={off} ldr={lr} roff={ro}")
    plan.destroy()
    W.free()


# ---- 3. yardstick (b): the existing call ----------------------------------------------------------------------------------

@pytest.mark.parametrize("K,N", [(300, 33), (2049, 260), (257, 130)])
def test_against_the_existing_call(gpu, oracle, env, K, N):
    """sgemm_i8 with the column scales into an fp32 Y0, then torch: Y0 + R for an fp32 Y, (Y0 + R.float()).to(bf16)
    for a bf16 one -- one rounding, which a bf16 Y0 followed by a bf16 add does not give."""
    torch = gpu
    c = case(torch, oracle, K, N)
    b = res_bias(c)
    env()
    W, plan = packed_plan(c["Wd"])
    q, s = c["q"]["bf16"], c["s"]["bf16"]
    twice = 0
    for M in DECODE_MS + GEMM_MS:
        Xq, Sd = torch.from_numpy(np.ascontiguousarray(q[:M])).to(DEV), dev_f32(torch, s[:M])
        Bd, Cd = dev_f32(torch, b), dev_f32(torch, c["Cs"])
        Y0 = torch.empty((M, N), device=DEV)
        plan.sgemm_i8(Xq, Sd, Bd, Y0, M, N, "basic", 0.0, col_scale=Cd)
        v = value(c, "q8b", M, c["Cs"], b)
        for ytype in YTYPES:
            dt = torch.float32 if ytype == "f32" else torch.bfloat16
            R = torch.from_numpy(r_values(torch, v, ytype, 31 * M + N)).to(DEV).to(dt)
            want = (Y0 + R.float()).to(dt)
            Y = torch.full((M, N + 1), SENT, dtype=dt, device=DEV)
            plan.sgemm_i8(Xq, Sd, Bd, Y, M, N + 1, "basic", 0.0, col_scale=Cd, residual=R, ldr=N)
            torch.cuda.synchronize()
            bits = torch.int32 if ytype == "f32" else torch.int16
            assert torch.equal(Y[:, :N].contiguous().view(bits), want.view(bits)), f"M={M} {ytype}"
            assert torch.all(Y[:, N] == SENT)
            if ytype == "bf16":
                twice += int((Y0.to(dt) + R != want).sum())
    assert twice > 0, "the twice-rounded composition differs somewhere: the header says so"
    plan.destroy()
    W.free()


# ---- 4. the norm in front ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,N", [(300, 33), (2049, 260)])
def test_the_norm_form(gpu, oracle, env, K, N):
    """sgemm_q8_norm with a residual equals rmsnorm_rows -> quantize_rows_i8 -> sgemm_i8 with the residual, Y and
    dScale, fused ($TCSC_QFUSE=1: k_decode8q's norm form) and not, on the decode and the MFMA route, and in place."""
    torch = gpu
    c = case(torch, oracle, K, N)
    b = res_bias(c)
    gamma = nc.gamma_of(K, 2600 + K)
    Gd = dev_f32(torch, gamma)
    env()
    W, plan = packed_plan(c["Wd"])
    n = 0
    for knob in (None, "1"):
        for M in (1, 4, 16, 40):
            env(TCSC_QFUSE=knob)
            assert plan.launch_info_q8_norm(M, "f32")[2] == (knob == "1" and M <= 16)
            for xt in XTYPES:
                for ytype in YTYPES:
                    X = dev_x(torch, c["X"][xt][:M], xt)
                    Xn = torch.empty((M, K), device=DEV)
                    tcsc_amd.rmsnorm_rows(X, Xn, M, K, Gd, EPS)
                    Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
                    S0 = torch.empty(M, device=DEV)
                    tcsc_amd.quantize_rows_i8(Xn, Xq, S0, M, K)
                    v = np.zeros((M, N), np.float32)
                    R = r_values(torch, v, ytype, 11 * M + n)
                    (ldy, off), (ldr, roff) = layouts(N)[n % 5], r_layout(N, n)
                    rb = fill(YBuf(torch, M, N, ldr, roff, ytype), r_bits(R, ytype))
                    ref = YBuf(torch, M, N, ldy, off, ytype)
                    Bd, Cd = dev_f32(torch, b), dev_f32(torch, c["Cs"])
                    plan.sgemm_i8(Xq, S0, Bd, ref.Y, M, ldy, "basic", 0.0, col_scale=Cd, residual=rb.Y, ldr=ldr)
                    for inplace in (False, True):
                        yb = fill(YBuf(torch, M, N, ldy, off, ytype), r_bits(R, ytype)) if inplace else YBuf(torch, M, N, ldy,
                                                                                                             off, ytype)
                        S = torch.full((M + 1,), 5.0, device=DEV)
                        Xs = torch.empty((M, K), dtype=torch.int8, device=DEV)
                        plan.sgemm_q8_norm(X, Xs, S, Bd, yb.Y, M, ldy, Gd, EPS, "basic", 0.0, col_scale=Cd,
                                           residual=yb.Y if inplace else rb.Y, ldr=ldy if inplace else ldr)
                        tag = f"QFUSE={knob} M={M} {xt} {ytype} inplace={inplace}"
                        yb.check(ref.values(), tag)
                        assert torch.equal(S[:M].view(torch.int32), S0.view(torch.int32)) and S[M] == 5.0, tag
                    rb.check(r_bits(R, ytype), "R was written")
                    n += 1
    plan.destroy()
    W.free()


# ---- 5. the same bits on every route ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,N", [(300, 33), (2049, 260)])
def test_equal_bits_across_routes(gpu, oracle, env, K, N):
    """The same q, s and R: k_decode8 at M = 16 against rows 0 .. 15 of an M = 17 call (k_gemm8w2), and a packed
    against an ordinary plan (k_gemm8)."""
    torch = gpu
    c = case(torch, oracle, K, N)
    b = res_bias(c)
    q, s = c["q"]["bf16"], c["s"]["bf16"]
    env()
    W, plan = packed_plan(c["Wd"])
    assert plan.launch_info_i8(16) == ("decode", 1) and plan.launch_info_i8(17)[0] == "mfma"
    Wo, other = ordinary_plan(env, c["Wd"])
    Bd, Cd = dev_f32(torch, b), dev_f32(torch, c["Cs"])

    def run(p, M, rows, R, ytype):
        Xq, Sd = torch.from_numpy(np.ascontiguousarray(q[:M])).to(DEV), dev_f32(torch, s[:M])
        rb = fill(YBuf(torch, M, N, N + 1, 1, ytype), r_bits(R[:M], ytype))
        yb = YBuf(torch, M, N, N, 0, ytype)
        p.sgemm_i8(Xq, Sd, Bd, yb.Y, M, N, "basic", 0.0, col_scale=Cd, residual=rb.Y, ldr=N + 1)
        return yb.values()[:rows]

    for ytype in YTYPES:
        R = r_values(torch, value(c, "q8b", 130, c["Cs"], b), ytype, 77)
        env()
        y16, y17 = run(plan, 16, 16, R, ytype), run(plan, 17, 16, R, ytype)
        np.testing.assert_array_equal(y16, y17, err_msg=f"decode against k_gemm8w2 {ytype}")
        np.testing.assert_array_equal(y16, add(value(c, "q8b", 16, c["Cs"], b), R[:16], ytype))
        for M in (40, 130):
            env()
            yp = run(plan, M, M, R, ytype)
            env(TCSC_PATH="mfma")
            assert other.launch_info_i8(M) == plan.launch_info_i8(M)
            np.testing.assert_array_equal(yp, run(other, M, M, R, ytype), err_msg=f"packed against ordinary M={M} {ytype}")
    plan.destroy()
    other.destroy()
    W.free()
    Wo.free()


# ---- 6. capture ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 40])
@pytest.mark.parametrize("ytype", YTYPES)
def test_a_captured_in_place_call_adds_once_per_replay(gpu, oracle, env, M, ytype):
    """After reserve(64): the in-place call captured on one stream and replayed three times equals yardstick (a)
    applied three times, and the plan holds what it held."""
    torch = gpu
    K, N = 300, 33
    c = case(torch, oracle, K, N)
    b = res_bias(c)
    env()
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan.packed(W)
    plan.reserve(64)
    held = plan.info()["device_bytes"]
    dt = torch.float32 if ytype == "f32" else torch.bfloat16
    X = dev_x(torch, c["X"]["bf16"][:M], "bf16")
    Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
    S, H = torch.zeros(M, device=DEV), torch.zeros((M, N), dtype=dt, device=DEV)
    Bd, Cd = dev_f32(torch, b), dev_f32(torch, c["Cs"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm_q8(X, Xq, S, Bd, H, M, N, "basic", 0.0, torch.cuda.current_stream().cuda_stream, col_scale=Cd,
                      residual=H)
    v = value(c, "q8b", M, c["Cs"], b)
    R = r_values(torch, v, ytype, 5 + M)
    R[np.abs(R) > 1e20] = 1.0  # three sums stay far from the largest bf16 value
    H.copy_(torch.from_numpy(R).to(DEV).to(dt))
    want = R
    for _ in range(3):
        torch.cuda.synchronize()
        g.replay()
        bits = add(v, want, ytype)
        want = bits.view(np.float32) if ytype == "f32" else (bits.astype(np.uint32) << 16).view(np.float32)
    torch.cuda.synchronize()
    got = H.view(torch.int32 if ytype == "f32" else torch.int16).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32 if ytype == "f32" else np.uint16), bits)
    assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()


# ---- 7. refusals on live plans ------------------------------------------------------------------------------------------------

def test_the_gather_and_small_routes_refuse_a_residual(gpu, oracle, env):
    """An ordinary plan made under $TCSC_PATH=gather: M = 40 routes to the gather and M = 2 to the gather or the
    small-M path; both entry points return TCSC_E_ARG naming the call and the path, and neither Y nor R is touched."""
    torch = gpu
    K, N = 300, 33
    c = case(torch, oracle, K, N)
    env(TCSC_PATH="gather")
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    plan = tcsc_amd.Plan(W)
    plan.reserve(40)
    Bd = dev_f32(torch, c["Bf"])
    for M in (40, 2):
        path = plan.launch_info_i8(M)[0]
        assert path in ("gather", "small") and plan.launch_info_q8(M, "f32")[0] == path
        name = {"gather": "gather", "small": "small-M"}[path]
        Xq, Sd = torch.from_numpy(c["q"]["f32"][:M].copy()).to(DEV), dev_f32(torch, c["s"]["f32"][:M])
        X = dev_x(torch, c["X"]["f32"][:M], "f32")
        for ytype in YTYPES:
            yb, rb = YBuf(torch, M, N, N, 0, ytype), YBuf(torch, M, N, N, 0, ytype)
            with pytest.raises(tcsc_amd.TcscError, match=rf"tcsc_gpu_sgemm_i8_res.*{name}"):
                plan.sgemm_i8(Xq, Sd, Bd, yb.Y, M, N, "basic", 0.0, residual=rb.Y)
            with pytest.raises(tcsc_amd.TcscError, match=rf"tcsc_gpu_sgemm_q8_res.*{name}"):
                plan.sgemm_q8(X, torch.empty_like(Xq), torch.empty(M, device=DEV), Bd, yb.Y, M, N, "basic", 0.0,
                              residual=rb.Y)
            assert yb.untouched() and rb.untouched(), "a refused call wrote Y or R"
    plan.destroy()
    W.free()


def test_a_live_plan_refuses_bad_residual_arguments(gpu, oracle, env):
    torch = gpu
    K, N, M = 300, 33, 4
    c = case(torch, oracle, K, N)
    env()
    W, plan = packed_plan(c["Wd"])
    X = dev_x(torch, c["X"]["f32"][:M], "f32")
    Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
    S, Bd = torch.empty(M, device=DEV), dev_f32(torch, c["Bf"])
    yb, rb = YBuf(torch, M, N, N + 3, 0, "f32"), YBuf(torch, M, N, N + 3, 0, "f32")
    i8 = lambda **kw: plan.sgemm_i8(Xq, S, Bd, yb.Y, M, N + 3, "basic", 0.0, **kw)
    q8 = lambda **kw: plan.sgemm_q8(X, Xq, S, Bd, yb.Y, M, N + 3, "basic", 0.0, **kw)
    for f, name in ((i8, "tcsc_gpu_sgemm_i8_res"), (q8, "tcsc_gpu_sgemm_q8_res")):
        with pytest.raises(tcsc_amd.TcscError, match=rf"{name}.*ldr"):
            f(residual=rb.Y, ldr=N - 1)
        with pytest.raises(tcsc_amd.TcscError, match=rf"{name}.*in place"):
            f(residual=yb.Y, ldr=N + 2)  # dR == dY with another pitch; ldr >= cols, so the earlier check passes
        with pytest.raises(tcsc_amd.TcscError, match=rf"{name}.*ldr"):
            f(residual=yb.Y, ldr=N - 1)  # both wrong: ldr < cols answers first
    # a NULL dR through the C interface (the Python keyword None means no residual)
    import ctypes as C

    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = tcsc_amd.lib().tcsc_gpu_sgemm_i8_res(plan.handle, vp(Xq), vp(S), None, vp(Bd), None, N, vp(yb.Y), 0, M, N + 3, None)
    assert rc == 1 and "NULL dR" in tcsc_amd.last_error()
    # the residual's dtype is Y's
    with pytest.raises(tcsc_amd.TcscError, match="dtype"):
        i8(residual=torch.zeros((M, N), dtype=torch.bfloat16, device=DEV))
    assert yb.untouched() and rb.untouched()
    plan.destroy()
    W.free()


# ---- 8. the layers -------------------------------------------------------------------------------------------------------------

def test_the_layer_takes_a_residual(gpu, oracle, env):
    torch = gpu
    from tcsc_amd.nn import PackedTernaryLinear

    K, N = 300, 33
    c = case(torch, oracle, K, N)
    env()
    gamma = nc.gamma_of(K, 2626)
    for norm in (False, True):
        kw = dict(norm_weight=gamma, norm_eps=EPS) if norm else {}
        f32 = PackedTernaryLinear(c["Wd"], c["Bf"], weight_scale=c["Cs"], **kw)
        b16 = PackedTernaryLinear(c["Wd"], c["Bf"], weight_scale=c["Cs"], out_dtype=torch.bfloat16, **kw)
        for M in (3, 40):
            x = dev_x(torch, c["X"]["bf16"][:M], "bf16")
            r = torch.from_numpy(r_values(torch, np.zeros((M, N), np.float32), "bf16", M)).to(DEV)
            y = f32(x, residual=r)
            assert y.dtype == torch.float32 and y.data_ptr() != r.data_ptr()
            assert torch.equal(y.view(torch.int32), (f32(x) + r).view(torch.int32)), f"fp32 M={M} norm={norm}"
            rb = r.to(torch.bfloat16)
            y = b16(x, residual=rb)
            want = (f32(x) + rb.float()).to(torch.bfloat16)  # the twin at out_dtype=float32: one rounding
            assert y.dtype == torch.bfloat16 and torch.equal(y.view(torch.int16), want.view(torch.int16)), f"bf16 M={M}"
            keep = rb.clone()
            out = b16(x, residual=rb, inplace=True)
            assert out is rb and torch.equal(rb.view(torch.int16), want.view(torch.int16))
            # a leading shape, and a residual with a row pitch
            x3, r3 = x.reshape(1, M, K), keep.reshape(1, M, N).clone()
            assert torch.equal(b16(x3, residual=r3).view(torch.int16), want.reshape(1, M, N).view(torch.int16))
            wide = torch.full((M, N + 5), SENT, dtype=torch.bfloat16, device=DEV)
            wide[:, :N] = keep
            out = b16(x, residual=wide[:, :N], inplace=True)
            assert out.data_ptr() == wide.data_ptr() and torch.equal(wide[:, :N].contiguous().view(torch.int16),
                                                                     want.view(torch.int16))
            assert torch.all(wide[:, N:] == SENT)
    x, r = dev_x(torch, c["X"]["f32"][:3], "f32"), torch.zeros((3, N), device=DEV)
    with pytest.raises(tcsc_amd.TcscError, match="PReLU"):
        PackedTernaryLinear(c["Wd"], c["Bf"], a=0.2)(x, residual=r)
    with pytest.raises(tcsc_amd.TcscError, match="residual"):
        b16(x, residual=r)  # an fp32 residual on a bf16 layer
    with pytest.raises(tcsc_amd.TcscError, match="shape"):
        f32(x, residual=torch.zeros((3, N + 1), device=DEV))
    with pytest.raises(tcsc_amd.TcscError, match="grad"):
        f32(x, residual=torch.zeros((3, N), device=DEV, requires_grad=True))
    with pytest.raises(tcsc_amd.TcscError, match="inplace"):
        f32(x, inplace=True)


def test_the_mlp_takes_a_residual(gpu, oracle, env):
    """PackedTernaryMLP with a residual equals its two layers composed by hand."""
    torch = gpu
    from tcsc_amd.nn import PackedTernaryGLU, PackedTernaryLinear, PackedTernaryMLP

    K, H = 300, 130
    env()
    Wg, Wu, Wd = (oracle.ternary(s, 0.6, 2630 + i) for i, s in enumerate(((K, H), (K, H), (H, K))))
    glu = PackedTernaryGLU(Wg, Wu, act="relu2", norm_eps=EPS, out_dtype=torch.bfloat16)
    down = PackedTernaryLinear(Wd, oracle.uniform((K,), 2640), out_dtype=torch.bfloat16, norm_eps=EPS)
    mlp = PackedTernaryMLP(glu, down)
    rng = np.random.default_rng(2641)
    for M in (2, 40):
        x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(DEV).to(torch.bfloat16)
        h = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(DEV).to(torch.bfloat16)
        want = down(glu(x), residual=h)
        assert torch.equal(mlp(x, residual=h).view(torch.int16), want.view(torch.int16))
        assert torch.equal(mlp(x).view(torch.int16), down(glu(x)).view(torch.int16))
        h2 = h.clone()
        assert mlp(x, residual=h2, inplace=True) is h2 and torch.equal(h2.view(torch.int16), want.view(torch.int16))
