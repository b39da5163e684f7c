"""The int8 calls at the edges of fp32, on every route: sums of 2^24 and more over a long K (group A), special values
through every tail of the epilogue (group B), and the quantizer's range (group C).  The inputs and the numpy
yardstick are tests/i8_edge_cases.py; tests/test_i8_edges_cases.py shows on the CPU that these inputs reach the edges
and that a kernel with a truncating float(S), a bf16 rounding without its NaN branch or the quantizer before tiny rows
were defined could not pass here.

Every case first asserts its route with launch_info_*; Y is compared as integer bits over its whole sentinel-filled
allocation (the YBuf of tests/test_gpu_out.py), a NaN for a NaN and the same bits everywhere else."""
import time

import numpy as np
import pytest

import i8_edge_cases as ec
import norm_cases as nc
import tcsc_amd
from test_gpu_out import DEV, KNOBS, YBuf, dev_f32, dev_x, ordinary_plan, packed_plan

pytestmark = pytest.mark.gpu

YTYPES = ("f32", "bf16")
EPS = nc.EPS


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
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


def layouts(N):
    """(ldy, off): an aligned base and a base one element in, ldy = N and N + 1."""
    return ((N, 0), (N + 1, 0), (N, 1), (N + 1, 1))


def check(yb, want, what):
    ec.assert_bits(yb.bits(), yb.expected(want), f"{what} (M={yb.M} N={yb.N} ldy={yb.ldy} off={yb.off} {yb.ytype}; flat "
                                                 f"index = off + row * ldy + column)")


def fill(yb, bits):
    """A YBuf with `bits` (M x N) in place and the sentinel elsewhere: a residual, bit for bit."""
    torch = yb.torch
    want = yb.expected(bits)
    if yb.ytype == "f32":
        yb.buf.view(torch.int32).copy_(torch.from_numpy(want.view(np.int32)).to(DEV))
    else:
        yb.buf.view(torch.int16).copy_(torch.from_numpy(want.view(np.int16)).to(DEV))
    return yb


def dev_bits(torch, v):
    """float32 values to the device, bit for bit."""
    return torch.from_numpy(np.ascontiguousarray(v, np.float32).view(np.int32).copy()).to(DEV).view(torch.float32)


def scales_of(torch, S, M):
    torch.cuda.synchronize()
    S = S.cpu().numpy()
    assert S[M] == 5.0
    return S[:M].view(np.uint32)


# ---- group A: sums of 2^24 and more, long K --------------------------------------------------------------------------------

def a_sweep(torch, plan, c, Xd, M, what, n=0):
    for call in ec.A_CALLS:
        s, cs, b, ytype = ec.a_operands(c, call)
        ldy, off = layouts(ec.A_N)[n % 4]
        n += 1
        yb = YBuf(torch, M, ec.A_N, ldy, off, ytype)
        plan.sgemm_i8(Xd[:M], None if s is None else dev_f32(torch, s[:M]), dev_f32(torch, b), yb.Y, M, ldy, "basic", 0.0,
                      col_scale=None if cs is None else dev_f32(torch, cs))
        check(yb, ec.a_expected(c, call, M), f"{what} M={M} {call}")
    return n


@pytest.mark.parametrize("K", ec.A_KS)
def test_group_a_float_of_a_large_sum(gpu, env, K):
    """float(S) is rounded to nearest even where |S| >= 2^24, on k_decode8 (M = 1, 16), k_decode8r (M = 24: two row
    tiles, M = 40: four), k_gemm8w2 with its K split and k_reduce_i8, and k_gemm8 on an ordinary plan; K = 133120 takes
    the 16-byte loads of X and 133121 the byte loads."""
    torch = gpu
    c = ec.group_a(K)
    Xd = torch.from_numpy(c["X"]).to(DEV)
    env()
    W, plan = packed_plan(c["Wd"], rows=ec.A_ROWS)
    n = 0
    for M in (1, 16):
        assert plan.launch_info_i8(M) == ("decode", 1)
        n = a_sweep(torch, plan, c, Xd, M, "k_decode8", n)
    plan.set_decode_rows(64)
    for M, rt in ((24, 2), (40, 4)):
        assert plan.launch_info_i8(M) == ("decode", 1) and plan.launch_info_decode(M)[0] == rt
        n = a_sweep(torch, plan, c, Xd, M, f"k_decode8r RT={rt}", n)
    plan.set_decode_rows(16)
    for M in (24, 40):
        path, slices = plan.launch_info_i8(M)
        assert path == "mfma" and slices > 1, (M, path, slices)
        n = a_sweep(torch, plan, c, Xd, M, f"k_gemm8w2, {slices} slices", n)
    env(TCSC_MFMA_WGS="0")
    assert plan.launch_info_i8(40) == ("mfma", 1)
    n = a_sweep(torch, plan, c, Xd, 40, "k_gemm8w2 unsplit", n)
    plan.destroy()
    W.free()
    t0 = time.perf_counter()
    Wo, other = ordinary_plan(env, c["Wd"], rows=ec.A_ROWS)
    print(f"ordinary plan of {K} x {ec.A_N}: {time.perf_counter() - t0:.2f} s")
    env(TCSC_PATH="mfma")
    for M in (24, 40):
        path, slices = other.launch_info_i8(M)
        assert path == "mfma", (M, path)
        n = a_sweep(torch, other, c, Xd, M, f"k_gemm8, {slices} slices", n)
    other.destroy()
    Wo.free()


# ---- group B: special values through every tail ------------------------------------------------------------------------------

class BCalls:
    """The calls of one shape of group B on one plan: every scene, Y type and layout on the first M rows of one input
    kind.  kinds: 'i8' (int8 X, the caller's row scales), 'q8f' / 'q8b' (fp32 / bf16 X through sgemm_q8), and with
    'n' / 'g' appended sgemm_q8_norm without / with gamma."""

    def __init__(self, torch, c):
        self.torch, self.c, self.n = torch, c, 0
        self.Xi = torch.from_numpy(c["Xi"]).to(DEV)
        self.Xf = {xt: dev_x(torch, c["Xf"], xt) for xt in ("f32", "bf16")}
        self.gamma = dev_f32(torch, c["gamma"])
        self.qs = {}

    def quantized(self, kind):
        """(S, scale) of the yardstick for a q8 kind."""
        tail = kind[3:]
        if tail not in self.qs:
            norm = None if tail == "" else (self.c["gamma"] if tail == "g" else None, EPS)
            _, s, S = ec.b_quantized(self.c, norm=norm)
            self.qs[tail] = (S, s)
        return self.qs[tail]

    def call(self, plan, kind, M, sc, yb, R=None, ldr=None):
        torch, c = self.torch, self.c
        Bd = dev_bits(torch, sc["b"])
        Cd = None if sc["c"] is None else dev_bits(torch, sc["c"])
        kw = dict(col_scale=Cd, residual=R, ldr=ldr) if R is not None else dict(col_scale=Cd)
        if kind == "i8":
            plan.sgemm_i8(self.Xi[:M], dev_bits(torch, sc["s"][:M]), Bd, yb.Y, M, yb.ldy, sc["variant"], sc["a"], **kw)
            return
        X = self.Xf["bf16" if kind[2] == "b" else "f32"][:M]
        Xq = torch.empty((M, c["K"]), dtype=torch.int8, device=DEV)
        S = torch.full((M + 1,), 5.0, device=DEV)
        if len(kind) == 3:
            plan.sgemm_q8(X, Xq, S, Bd, yb.Y, M, yb.ldy, sc["variant"], sc["a"], **kw)
        else:
            plan.sgemm_q8_norm(X, Xq, S, Bd, yb.Y, M, yb.ldy, self.gamma if kind[3] == "g" else None, EPS, sc["variant"],
                               sc["a"], **kw)
        ec.assert_bits(scales_of(torch, S, M), ec.bits32(self.quantized(kind)[1][:M]), f"{kind} M={M}: scales")

    def sweep(self, plan, kind, M, what):
        torch, c, N = self.torch, self.c, self.c["N"]
        base = "i8" if kind == "i8" else "q8"
        qs = None if kind == "i8" else self.quantized(kind)
        for name, sc in ec.b_scenes(c, base).items():
            for ytype in YTYPES:
                _, want, R = ec.b_expected(c, base, sc, M, ytype, qs)
                for ldy, off in layouts(N):
                    tag = f"{what} {kind} M={M} scene '{name}'"
                    self.n += 1
                    if R is None:
                        yb = YBuf(torch, M, N, ldy, off, ytype)
                        self.call(plan, kind, M, sc, yb)
                        check(yb, want, tag)
                        continue
                    ldr, roff = layouts(N)[(self.n + 1) % 4]  # R's alignment and pitch rotate against Y's
                    rb = fill(YBuf(torch, M, N, ldr, roff, ytype), ec.rbits(R, ytype))
                    yb = YBuf(torch, M, N, ldy, off, ytype)
                    self.call(plan, kind, M, sc, yb, rb.Y, ldr)
                    check(yb, want, tag + f" ldr={ldr} roff={roff}")
                    ec.assert_bits(rb.bits(), rb.expected(ec.rbits(R, ytype)), tag + ": R was written")
                    ib = fill(YBuf(torch, M, N, ldy, off, ytype), ec.rbits(R, ytype))
                    self.call(plan, kind, M, sc, ib, ib.Y, ldy)
                    check(ib, want, tag + " in place")


ROUTES = ("k_decode8q", "k_decode8q norm", "k_decode8", "k_decode8 QFUSE=0", "k_decode8r", "k_gemm8w2", "k_gemm8")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("K", ec.B_KS)
def test_group_b_special_values(gpu, env, K, route):
    """+-0, +-inf, NaNs, subnormals, the bf16 ties and the values that round to bf16 inf, placed in s, c, b, a and R and
    followed to Y: both Y types, aligned and unaligned bases, ldy = N and N + 1, out of place and in place.  K = 2049
    splits by the default rule on the MFMA routes, so k_reduce_i8 finishes those calls (the smallest slice of the int8
    GEMM is 512 k: the two smaller K never split)."""
    torch = gpu
    c = ec.group_b(K)
    calls = BCalls(torch, c)
    env()
    if route == "k_gemm8":
        W, plan = ordinary_plan(env, c["Wd"], rows=ec.B_ROWS)
        env(TCSC_PATH="mfma")
        for M in (40, 65):
            path, slices = plan.launch_info_i8(M)
            assert path == "mfma" and (slices > 1) == (K == 2049), (M, path, slices)
            assert plan.launch_info_q8(M, "f32") == ("mfma", slices, False)
            calls.sweep(plan, "i8", M, route)
            calls.sweep(plan, "q8f", M, route)
    else:
        W, plan = packed_plan(c["Wd"], rows=ec.B_ROWS)
        if route == "k_decode8q":
            for M in (1, 4):
                for kind in ("q8f", "q8b"):
                    assert plan.launch_info_q8(M, "bf16" if kind[2] == "b" else "f32") == ("decode", 1, True)
                    calls.sweep(plan, kind, M, route)
        elif route == "k_decode8q norm":
            env(TCSC_QFUSE="1")
            for M in (1, 4):
                for kind in ("q8fn", "q8bg", "q8fg", "q8bn"):
                    assert plan.launch_info_q8_norm(M, "bf16" if kind[2] == "b" else "f32") == ("decode", 1, True)
                    calls.sweep(plan, kind, M, route)
        elif route == "k_decode8":
            for M in (5, 16):
                assert plan.launch_info_i8(M) == ("decode", 1) and plan.launch_info_q8(M, "bf16") == ("decode", 1, False)
                calls.sweep(plan, "i8", M, route)
                calls.sweep(plan, "q8b", M, route)
        elif route == "k_decode8 QFUSE=0":
            env(TCSC_QFUSE="0")
            for M in (1, 4):
                assert plan.launch_info_q8(M, "f32") == ("decode", 1, False) and plan.launch_info_i8(M) == ("decode", 1)
                calls.sweep(plan, "q8f", M, route)
                calls.sweep(plan, "i8", M, route)
        elif route == "k_decode8r":
            plan.set_decode_rows(64)
            for M, rt in ((24, 2), (40, 4)):
                assert plan.launch_info_i8(M) == ("decode", 1) and plan.launch_info_decode(M)[0] == rt
                assert plan.launch_info_q8(M, "f32") == ("decode", 1, False)
                calls.sweep(plan, "i8", M, f"{route} RT={rt}")
                calls.sweep(plan, "q8f", M, f"{route} RT={rt}")
        else:
            assert plan.decode_rows == 16
            for M in (40, 65):
                path, slices = plan.launch_info_i8(M)
                assert path == "mfma" and (slices > 1) == (K == 2049), (M, path, slices)  # 2049: k_reduce_i8 finishes
                calls.sweep(plan, "i8", M, f"{route}, {slices} slices")
                calls.sweep(plan, "q8b", M, f"{route}, {slices} slices")
    plan.destroy()
    W.free()


def gated_plans(c):
    Ws = [tcsc_amd.TcscMatrix.from_dense(Wd) for Wd in (c["Wd"], np.ascontiguousarray(c["Wd"][:, ::-1]))]
    ps = [tcsc_amd.Plan.packed(W) for W in Ws]
    ps[0].reserve(ec.B_ROWS)
    return Ws, ps


@pytest.mark.parametrize("K", ec.B_KS)
def test_group_b_gated(gpu, env, K):
    """The gated call on the decode (M = 4) and the MFMA route (M = 40): relu2 with g and u from the table, and SiLU at
    the g where expf(-g) is exactly 0, 1, inf or NaN -- g = -inf gives -inf / inf = NaN."""
    torch = gpu
    c = ec.group_b(K)
    N = c["N"]
    env()
    Ws, (gate, up) = gated_plans(c)
    Xi = torch.from_numpy(c["Xi"]).to(DEV)
    n = 0
    for M in (4, 40):
        path, slices, fused = tcsc_amd.launch_info_glu(gate, up, M, "f32")
        assert path == ("decode" if M == 4 else "mfma") and (slices > 1) == (M == 40 and K == 2049), (M, path, slices)
        for act in ("relu2", "silu"):
            Sg, Su, s, cg, bg, cu, bu = ec.b_glu_operands(c, act, M)
            g, u = ec.i8_value(Sg, s, cg, bg), ec.i8_value(Su, s, cu, bu)
            h = ec.relu2(g, u) if act == "relu2" else ec.silu_exact(g, u)
            Xd = Xi[:M] if act == "relu2" else torch.zeros((M, K), dtype=torch.int8, device=DEV)
            for ytype in YTYPES:
                for ldy, off in layouts(N):
                    yb = YBuf(torch, M, N, ldy, off, ytype)
                    tcsc_amd.sgemm_i8_glu(gate, up, Xd, dev_bits(torch, s), dev_bits(torch, bg), dev_bits(torch, bu), yb.Y, M,
                                          ldy, act, None if cg is None else dev_bits(torch, cg),
                                          None if cu is None else dev_bits(torch, cu))
                    check(yb, ec.ybits(h, ytype), f"i8 glu {act} M={M} ({path}, {slices} slices)")
                    n += 1
        # the float X through the quantizer (fused at M = 4: k_decode8qg), relu2 with the table in the biases
        _, _, _, cg, bg, cu, bu = ec.b_glu_operands(c, "relu2", M)
        Sf_up = ec.int_sums(c["qf"], c["Wd"][:, ::-1])
        g, u = ec.i8_value(c["Sf"][:M], c["sf"][:M], cg, bg), ec.i8_value(Sf_up[:M], c["sf"][:M], cu, bu)
        for xt in ("f32", "bf16"):
            for ytype in YTYPES:
                ldy, off = layouts(N)[n % 4]
                n += 1
                yb = YBuf(torch, M, N, ldy, off, ytype)
                S = torch.full((M + 1,), 5.0, device=DEV)
                Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
                tcsc_amd.sgemm_q8_glu(gate, up, dev_x(torch, c["Xf"][:M], xt), Xq, S, dev_bits(torch, bg), dev_bits(torch, bu),
                                      yb.Y, M, ldy, "relu2", dev_bits(torch, cg), None)
                ec.assert_bits(scales_of(torch, S, M), ec.bits32(c["sf"][:M]), "glu scales")
                check(yb, ec.ybits(ec.relu2(g, u), ytype), f"q8 glu relu2 {xt} M={M}")
    for p in (gate, up):
        p.destroy()
    for W in Ws:
        W.free()


@pytest.mark.parametrize("K", ec.B_KS)
def test_group_b_grouped(gpu, env, K):
    """Two members on one X, decode (M = 4) and MFMA (M = 40): one carries the table in c and b, the other is
    ordinary, and the ordinary member's bits are those of its stand-alone call."""
    torch = gpu
    c = ec.group_b(K)
    N, N2 = c["N"], 33
    env()
    W2d = np.ascontiguousarray(c["Wd"][:, 2:2 + N2])
    Ws = [tcsc_amd.TcscMatrix.from_dense(c["Wd"]), tcsc_amd.TcscMatrix.from_dense(W2d)]
    plans = [tcsc_amd.Plan.packed(W) for W in Ws]
    for p in plans:
        p.reserve(ec.B_ROWS)
    Xi = torch.from_numpy(c["Xi"]).to(DEV)
    b2, c2 = c["b"][:N2], c["c"][:N2]
    S2 = ec.int_sums(c["Xi"], W2d)
    for M in (4, 40):
        path, slices, fused = tcsc_amd.launch_info_group(plans, M, "f32")
        assert path == ("decode" if M == 4 else "mfma"), (M, path, slices)
        for shift, ctab in ((0, False), (9, True)):
            b1 = ec.table_at(N, shift)
            c1 = ec.table_at(N, shift + 20) if ctab else c["c"]
            for ytype in YTYPES:
                for ldy, off in layouts(N):
                    y1, y2 = YBuf(torch, M, N, ldy, off, ytype), YBuf(torch, M, N2, N2 + off, off, ytype)
                    Sd = dev_bits(torch, c["s"][:M])
                    tcsc_amd.sgemm_i8_group(plans, Xi[:M], Sd, [dev_bits(torch, b1), dev_bits(torch, b2)], [y1.Y, y2.Y], M,
                                            [ldy, N2 + off], [dev_bits(torch, c1), dev_bits(torch, c2)])
                    tag = f"group M={M} ({path}) table in {'c and b' if ctab else 'b'}"
                    check(y1, ec.ybits(ec.i8_value(c["Si"][:M], c["s"][:M], c1, b1), ytype), tag + ": the table's member")
                    check(y2, ec.ybits(ec.i8_value(S2[:M], c["s"][:M], c2, b2), ytype), tag + ": the ordinary member")
                    alone = YBuf(torch, M, N2, N2 + off, off, ytype)
                    plans[1].sgemm_i8(Xi[:M], Sd, dev_bits(torch, b2), alone.Y, M, N2 + off, "basic", 0.0,
                                      col_scale=dev_bits(torch, c2))
                    assert np.array_equal(y2.bits(), alone.bits()), tag + ": the ordinary member against its own call"
        # the float X through the quantizer (fused at M = 4: k_decode8qm)
        S2f = ec.int_sums(c["qf"], W2d)
        b1 = ec.table_at(N, 4)
        for xt in ("f32", "bf16"):
            for ytype in YTYPES:
                y1, y2 = YBuf(torch, M, N, N + 1, 1, ytype), YBuf(torch, M, N2, N2, 0, ytype)
                S = torch.full((M + 1,), 5.0, device=DEV)
                Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
                tcsc_amd.sgemm_q8_group(plans, dev_x(torch, c["Xf"][:M], xt), Xq, S, [dev_bits(torch, b1), dev_bits(torch, b2)],
                                        [y1.Y, y2.Y], M, [N + 1, N2], [dev_bits(torch, c["c"]), dev_bits(torch, c2)])
                ec.assert_bits(scales_of(torch, S, M), ec.bits32(c["sf"][:M]), "group scales")
                check(y1, ec.ybits(ec.i8_value(c["Sf"][:M], c["sf"][:M], c["c"], b1), ytype), f"q8 group {xt} M={M}")
                check(y2, ec.ybits(ec.i8_value(S2f[:M], c["sf"][:M], c2, b2), ytype), f"q8 group {xt} M={M}: ordinary")
    for p in plans:
        p.destroy()
    for W in Ws:
        W.free()


# ---- group C: the quantizer's range -------------------------------------------------------------------------------------------

def quantize(torch, X, xt, M, K, norm=None):
    """quantize_rows_i8 (norm: quantize_rows_i8_norm with (gamma or None, eps)) -> (q int8, scale bits)."""
    Xd = dev_x(torch, X[:M], xt) if not isinstance(X, torch.Tensor) else X
    Xq = torch.full((M + 1, K), 77, dtype=torch.int8, device=DEV)
    S = torch.full((M + 1,), 5.0, device=DEV)
    if norm is None:
        tcsc_amd.quantize_rows_i8(Xd, Xq, S, M, K)
    else:
        tcsc_amd.quantize_rows_i8_norm(Xd, Xq, S, M, K, None if norm[0] is None else dev_f32(torch, norm[0]), norm[1])
    s = scales_of(torch, S, M)
    q = Xq.cpu().numpy()
    assert np.all(q[M] == 77)
    return q[:M], s


def dev_x_bits(torch, X, xt):
    """fp32 values (bf16: values that are bf16 values) to the device bit for bit, non-finite ones included."""
    t = dev_bits(torch, X)
    if xt == "f32":
        return t
    assert not np.any(ec.bits32(X) & 0xFFFF)
    return (t.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)


@pytest.mark.parametrize("K", ec.C_KS)
def test_group_c_quantize_rows(gpu, env, K):
    """quantize_rows_i8 on fp32 and bf16 rows whose maxima stand on either side of the largest amax with
    fl(127 / amax) = inf, on subnormal maxima, on FLT_MAX and 3e38; quantize_rows_i8_norm on the rows without those two."""
    torch = gpu
    env()
    c = ec.group_c(K)
    for xt in ("f32", "bf16"):
        q, s, _ = ec.c_expected(c, xt)
        gq, gs = quantize(torch, c["X"][xt], xt, ec.C_ROWS, K)
        ec.assert_bits(gs, ec.bits32(s), f"quantize_rows_i8 {xt} K={K}: scale")
        bad = np.flatnonzero((gq != q).any(1))
        assert not bad.size, (f"quantize_rows_i8 {xt} K={K}: Xq differs in rows {list(bad)} "
                              f"({[c['names'][m] for m in bad]}); row {bad[0]}: got {gq[bad[0]][:8]}, expected {q[bad[0]][:8]}")
    c = ec.group_c(K, big=False)
    for xt in ("f32", "bf16"):
        for gamma in (None, c["gamma"]):
            q, s, _ = ec.c_expected(c, xt, (gamma, EPS))
            gq, gs = quantize(torch, c["X"][xt], xt, ec.C_ROWS, K, (gamma, EPS))
            ec.assert_bits(gs, ec.bits32(s), f"quantize_rows_i8_norm {xt} K={K} gamma={gamma is not None}: scale")
            assert np.array_equal(gq, q), f"quantize_rows_i8_norm {xt} K={K} gamma={gamma is not None}: Xq"


def c_run_q8(torch, plan, c, Xd, M, ytype, n, norm=None):
    """sgemm_q8 (norm: sgemm_q8_norm) on device rows Xd -> (YBuf, scale bits, Xq)."""
    ldy, off = layouts(ec.C_N)[n % 4]
    yb = YBuf(torch, M, ec.C_N, ldy, off, ytype)
    Xq = torch.full((M, c["K"]), 77, dtype=torch.int8, device=DEV)
    S = torch.full((M + 1,), 5.0, device=DEV)
    if norm is None:
        plan.sgemm_q8(Xd, Xq, S, dev_f32(torch, c["b"]), yb.Y, M, ldy, "basic", 0.0)
    else:
        plan.sgemm_q8_norm(Xd, Xq, S, dev_f32(torch, c["b"]), yb.Y, M, ldy, None if norm[0] is None else dev_f32(torch, norm[0]),
                           norm[1], "basic", 0.0)
    return yb, scales_of(torch, S, M), Xq.cpu().numpy()


@pytest.mark.parametrize("K", ec.C_KS)
def test_group_c_sgemm_q8(gpu, env, K):
    """sgemm_q8 fused (M = 1, 4) and unfused (M = 16; 40 at both decode-rows settings), sgemm_q8_glu and sgemm_q8_group
    at M = 4: Xq (where the call writes it), the scales and Y equal the restatement."""
    torch = gpu
    c = ec.group_c(K)
    env()
    W, plan = packed_plan(c["Wd"], rows=ec.C_ROWS)
    n = 0
    for M, knob, rows, fused in ((1, "1", 16, True), (4, "1", 16, True), (4, "0", 16, False), (16, None, 16, False),
                                 (16, "1", 16, True), (40, None, 16, False), (40, None, 64, False)):
        env(TCSC_QFUSE=knob)
        plan.set_decode_rows(rows)
        for xt in ("f32", "bf16"):
            want_path = "mfma" if (M, rows) == (40, 16) else "decode"
            info = plan.launch_info_q8(M, xt)
            assert info[0] == want_path and info[2] == fused, (M, knob, rows, info)
            q, s, S = ec.c_expected(c, xt)
            for ytype in YTYPES:
                yb, gs, gq = c_run_q8(torch, plan, c, dev_x(torch, c["X"][xt][:M], xt), M, ytype, n)
                n += 1
                tag = f"sgemm_q8 K={K} M={M} {xt} QFUSE={knob} decode_rows={rows}"
                ec.assert_bits(gs, ec.bits32(s[:M]), tag + ": scale")
                check(yb, ec.ybits(ec.i8_value(S[:M], s[:M], None, c["b"]), ytype), tag)
                assert np.array_equal(gq, q[:M]) if not fused else np.all(gq == 77), tag + ": Xq"
    env(TCSC_QFUSE="1")
    plan.set_decode_rows(16)
    cn = ec.group_c(K, big=False)
    for M in (1, 4):
        for xt in ("f32", "bf16"):
            for gamma in (None, cn["gamma"]):
                assert plan.launch_info_q8_norm(M, xt) == ("decode", 1, True)
                q, s, S = ec.c_expected(cn, xt, (gamma, EPS))
                yb, gs, _ = c_run_q8(torch, plan, cn, dev_x(torch, cn["X"][xt][:M], xt), M, "f32", n, (gamma, EPS))
                n += 1
                ec.assert_bits(gs, ec.bits32(s[:M]), f"sgemm_q8_norm K={K} M={M} {xt}: scale")
                check(yb, ec.ybits(ec.i8_value(S[:M], s[:M], None, cn["b"]), "f32"), f"sgemm_q8_norm K={K} M={M} {xt}")
    # the gated and the grouped call at M = 4 (fused by the rule or not: the bits are the same)
    env()
    W2 = tcsc_amd.TcscMatrix.from_dense(np.ascontiguousarray(c["Wd"][:, ::-1]))
    up = tcsc_amd.Plan.packed(W2)
    M = 4
    for xt in ("f32", "bf16"):
        q, s, S = ec.c_expected(c, xt)
        Su = ec.int_sums(q, c["Wd"][:, ::-1])
        g, u = ec.i8_value(S[:M], s[:M], None, c["b"]), ec.i8_value(Su[:M], s[:M], None, c["b"][::-1])
        for ytype in YTYPES:
            yb = YBuf(torch, M, ec.C_N, ec.C_N + 1, 1, ytype)
            Sd = torch.full((M + 1,), 5.0, device=DEV)
            Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
            tcsc_amd.sgemm_q8_glu(plan, up, dev_x(torch, c["X"][xt][:M], xt), Xq, Sd, dev_f32(torch, c["b"]),
                                  dev_f32(torch, c["b"][::-1]), yb.Y, M, ec.C_N + 1, "relu2")
            ec.assert_bits(scales_of(torch, Sd, M), ec.bits32(s[:M]), f"sgemm_q8_glu K={K} {xt}: scale")
            check(yb, ec.ybits(ec.relu2(g, u), ytype), f"sgemm_q8_glu K={K} {xt}")
            y1, y2 = YBuf(torch, M, ec.C_N, ec.C_N, 0, ytype), YBuf(torch, M, ec.C_N, ec.C_N + 1, 1, ytype)
            Sd = torch.full((M + 1,), 5.0, device=DEV)
            tcsc_amd.sgemm_q8_group([plan, up], dev_x(torch, c["X"][xt][:M], xt), Xq, Sd,
                                    [dev_f32(torch, c["b"]), dev_f32(torch, c["b"][::-1])], [y1.Y, y2.Y], M, [ec.C_N, ec.C_N + 1])
            ec.assert_bits(scales_of(torch, Sd, M), ec.bits32(s[:M]), f"sgemm_q8_group K={K} {xt}: scale")
            check(y1, ec.ybits(g, ytype), f"sgemm_q8_group K={K} {xt}: member 0")
            check(y2, ec.ybits(u, ytype), f"sgemm_q8_group K={K} {xt}: member 1")
    up.destroy()
    W2.free()
    plan.destroy()
    W.free()


@pytest.mark.parametrize("K", ec.C_KS)
def test_group_c_nonfinite_rows_touch_no_other_row(gpu, env, K):
    """Rows holding inf or NaN between finite rows (M = 16 and 40): their own outputs are unspecified and not
    compared; every other row's Xq, scale and Y are those of the restatement, which are those of the call without them."""
    torch = gpu
    c = ec.group_c(K)
    env()
    W, plan = packed_plan(c["Wd"], rows=ec.C_ROWS)
    n = 0
    for M, knob, rows in ((16, None, 16), (16, "1", 16), (40, None, 16), (40, None, 64)):
        env(TCSC_QFUSE=knob)
        plan.set_decode_rows(rows)
        for xt in ("f32", "bf16"):
            X = ec.with_nonfinite_rows(c["X"][xt][:M])
            keep = np.isfinite(X).all(1)
            assert 0 < np.count_nonzero(~keep) < M and keep[0] and keep[M - 1]
            Xd = dev_x_bits(torch, X, xt)
            q, s, S = ec.c_expected(c, xt)
            tag = f"K={K} M={M} {xt} QFUSE={knob} decode_rows={rows}"
            gq, gs = quantize(torch, Xd, xt, M, K)
            assert np.array_equal(gq[keep], q[:M][keep]) and np.array_equal(gs[keep], ec.bits32(s[:M])[keep]), tag
            for ytype in YTYPES:
                yb, gs, gq = c_run_q8(torch, plan, c, Xd, M, ytype, n)
                n += 1
                want = ec.ybits(ec.i8_value(S[:M], s[:M], None, c["b"]), ytype)
                got = yb.values()
                assert np.array_equal(gs[keep], ec.bits32(s[:M])[keep]), tag + ": scale"
                ec.assert_bits(got[keep], want[keep], tag + f" {ytype}: Y of the finite rows")
                if knob != "1":
                    assert np.array_equal(gq[keep], q[:M][keep]), tag + ": Xq"
                # nothing outside Y's M x N was written, whatever the non-finite rows hold
                full = yb.expected(got)
                assert np.array_equal(yb.bits(), full), tag + ": a write outside Y"
    plan.destroy()
    W.free()
