"""tcsc_gpu_sgemm_i8_glu / tcsc_gpu_sgemm_q8_glu: Y = act(X Wg) * (X Wu) in the int8 call, on every
kernel that finishes one: k_decode8g, k_decode8qg (plain and norm form), the gated k_gemm8w2 and the gated k_reduce_i8
in its 4-column and scalar forms.

TCSC_GLU_RELU2 is an equality of bits against two yardsticks, neither of them the code under test:
  (a) numpy: the quantizer (and the norm) restated in float32, the exact integer sums, then in float32, one rounded
      operation per step,  g = fl(fl(fl(float(Sg) s) cg) + bg), u likewise, r = g < 0 ? 0 : g, h = fl(fl(r r) u), and
      for a bf16 Y the rounding restated on the uint32 bits;
  (b) the existing entry points: sgemm_i8 twice into fp32, then torch in fp32, relu(g).square() * u (and
      .to(bfloat16)).  (b) is evaluated once per shape and input kind on all ROWS rows and asserted equal to (a) there,
      so every gated result that equals (a) equals (b).
Y is compared as the whole sentinel-filled allocation (the YBuf of tests/test_gpu_out.py), and so is dG: untouched on
the decode route, and on the MFMA route the fp32 gate values on rows < M, columns < H, the sentinel elsewhere.

TCSC_GLU_SILU: the same bits on every route (decode fused, decode unfused, MFMA, MFMA split), and against fp64
evaluated on the fp32 g and u of yardstick (b) the bound of §24:
    |h - h64| <= SILU_REL |h64| + 2^-126,   SILU_REL = 2 (2^-23 + 3 2^-24) = 5 2^-23
-- the math library's expf is documented at 1 ulp (a relative 2^-23, which the sum 1 + e passes on scaled by
e / (1 + e) < 1), the add, the IEEE division and the multiply round to nearest (2^-24 each), first order, with a factor
2 of margin; 2^-126 covers results below the normal range.  The bound is derived, not fitted."""
import ctypes as C

import numpy as np
import pytest

import norm_cases as nc
import tcsc_amd
from test_gpu_out import DEV, KNOBS, YBuf, col_scales, dev_f32, dev_x, int_sums, layouts, np_bf16_bits, np_quantize
from test_gpu_out import ordinary_plan

pytestmark = pytest.mark.gpu

HS = (1, 15, 16, 17, 33, 130)
KS = (16, 257, 300, 2049)
DECODE_MS = (1, 2, 4, 5, 16)
GEMM_MS = (17, 33, 130)
ROWS = 130
YTYPES = ("f32", "bf16")
KINDS = ("i8s", "i8n", "q8f", "q8b", "q8fn", "q8bn")  # int8 X with / without row scales; fp32 / bf16 X; with the norm
SENT = 7.0
EPS = 1e-5
SILU_REL = 5.0 * 2.0 ** -23


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


# ---- yardstick (a) ------------------------------------------------------------------------------------------------------

def np_i8_out(S, s, c, b):
    v = S.astype(np.float32)
    if s is not None:
        v = v * np.asarray(s, np.float32)[:, None]
    if c is not None:
        v = v * np.asarray(c, np.float32)[None, :]
    v = v + np.asarray(b, np.float32)[None, :]
    assert v.dtype == np.float32
    return v


def np_relu2(g, u):
    r = np.where(g < 0, np.float32(0), g)
    h = (r * r) * u
    assert h.dtype == np.float32
    return h


def ybits(h, ytype):
    return np_bf16_bits(h) if ytype == "bf16" else np.ascontiguousarray(h, np.float32).view(np.uint32)


_cases = {}


def case(torch, o, K, H, rows=ROWS):
    """Wg, Wu, `rows` rows of X, and per input kind the numpy quantization (after the numpy norm where the kind has one)
    with the exact sums against both matrices; biases that make g cross zero and two different sets of column
    scales.  Computed once per shape and left unchanged; a test of M rows uses the first M."""
    key = (K, H, rows)
    if key in _cases:
        return _cases[key]
    seed = 24000 + 3 * K + 5 * H
    rng = np.random.default_rng(seed)
    c = dict(Wg=o.ternary((K, H), 0.67, seed), Wu=o.ternary((K, H), 0.6, seed + 1))
    X = (rng.standard_normal((rows, K)) * rng.choice([1e-2, 1.0, 37.0], (rows, 1))).astype(np.float32)
    X[2] = 0.0  # a row of zeros: scale 0, g = bg
    Xb = torch.from_numpy(X).to(torch.bfloat16).to(torch.float32).numpy()
    c["gamma"] = nc.gamma_of(K, seed + 2)
    c["X"] = {"f32": X, "bf16": Xb}
    c["cg"], c["cu"] = col_scales(H, seed + 3), col_scales(H, seed + 4)[::-1].copy()
    c["q"], c["s"], c["Sg"], c["Su"] = {}, {}, {}, {}
    for kind in KINDS:
        if kind.startswith("i8"):
            q, s = np_quantize(X)
            if kind == "i8n":
                s = None
            elif kind == "i8s":
                s = (s * np.float32(0.75)).astype(np.float32)  # fixed scales of the caller's, not the quantizer's
        else:
            x = c["X"]["bf16" if kind[2] == "b" else "f32"]
            if kind.endswith("n"):
                x = nc.np_rmsnorm(x, c["gamma"], EPS)[0]
            q, s = np_quantize(x)
        c["q"][kind], c["s"][kind] = q, s
        c["Sg"][kind], c["Su"][kind] = int_sums(q, c["Wg"]), int_sums(q, c["Wu"])
    # g crosses zero: the biases are of the size of the values they are added to, either sign
    g0 = np_i8_out(c["Sg"]["q8f"], c["s"]["q8f"], None, np.zeros(H, np.float32))
    mag = np.float32(np.median(np.abs(g0)) + 0.5)
    c["bg"] = (rng.uniform(-1, 1, H) * mag).astype(np.float32)
    c["bu"] = (rng.uniform(-1, 1, H) * np.float32(2.0)).astype(np.float32)
    _cases[key] = c
    return c


def gu(c, kind, cs, M=None):
    """The fp32 g and u of yardstick (a) on the first M rows (None: all); cs: the column scales set or NULL."""
    s = None if c["s"][kind] is None else c["s"][kind][:M]
    g = np_i8_out(c["Sg"][kind][:M], s, c["cg"] if cs else None, c["bg"])
    u = np_i8_out(c["Su"][kind][:M], s, c["cu"] if cs else None, c["bu"])
    return g, u


# ---- the plans and the calls ----------------------------------------------------------------------------------------------

class Plans:
    def __init__(self, c, packed=True, env=None, rows=ROWS):
        self.W, self.p = [], []
        for Wd in (c["Wg"], c["Wu"]):
            if packed:
                W = tcsc_amd.TcscMatrix.from_dense(Wd)
                p = tcsc_amd.Plan.packed(W)
            else:
                W, p = ordinary_plan(env, Wd, rows)
            self.W.append(W)
            self.p.append(p)
        if self.ok:
            self.gate.reserve(rows)

    ok = property(lambda self: all(p is not None for p in self.p))
    gate = property(lambda self: self.p[0])
    up = property(lambda self: self.p[1])

    def free(self):
        for p in self.p:
            if p is not None:
                p.destroy()
        for W in self.W:
            W.free()


class GBuf:
    """dG: a sentinel-filled M + 1 rows of pitch H (8 spare elements behind), or None."""

    def __init__(self, torch, M, H):
        self.torch, self.M, self.H = torch, M, H
        self.buf = torch.full(((M + 1) * H + 8,), SENT, dtype=torch.float32, device=DEV)

    def check(self, g, what):
        """g: the expected fp32 gate values (M x H), or None for an untouched buffer."""
        self.torch.cuda.synchronize()
        got = self.buf.cpu().numpy().view(np.uint32)
        want = np.full(got.shape, np.float32(SENT).view(np.uint32), np.uint32)
        if g is not None:
            want[:self.M * self.H] = np.ascontiguousarray(g, np.float32).view(np.uint32).reshape(-1)
        bad = np.flatnonzero(got != want)
        assert not bad.size, f"{what}: dG differs at element {int(bad[0])} ({bad.size} elements)"


def run(torch, pl, c, kind, M, H, ldy, off, ytype, cs, act, G="sentinel"):
    """One gated call on the first M rows; returns (YBuf, GBuf or None).  The scales a q8 call writes are checked
    against the numpy quantizer's here."""
    yb = YBuf(torch, M, H, ldy, off, ytype)
    gb = GBuf(torch, M, H) if G == "sentinel" else None
    Gd = gb.buf if gb is not None else G
    bg, bu = dev_f32(torch, c["bg"]), dev_f32(torch, c["bu"])
    cg = dev_f32(torch, c["cg"]) if cs else None
    cu = dev_f32(torch, c["cu"]) if cs else None
    if kind.startswith("i8"):
        Xq = torch.from_numpy(np.ascontiguousarray(c["q"][kind][:M])).to(DEV)
        Sd = None if c["s"][kind] is None else dev_f32(torch, c["s"][kind][:M])
        tcsc_amd.sgemm_i8_glu(pl.gate, pl.up, Xq, Sd, bg, bu, yb.Y, M, ldy, act, cg, cu, Gd)
    else:
        xt = "bf16" if kind[2] == "b" else "f32"
        X = dev_x(torch, c["X"][xt][:M], xt)
        Xq = torch.empty((M, X.shape[1]), dtype=torch.int8, device=DEV)
        S = torch.full((M + 1,), 5.0, device=DEV)
        norm = kind.endswith("n")
        tcsc_amd.sgemm_q8_glu(pl.gate, pl.up, X, Xq, S, bg, bu, yb.Y, M, ldy, act, cg, cu,
                              dev_f32(torch, c["gamma"]) if norm else None, EPS if norm else None, Gd)
        torch.cuda.synchronize()
        S = S.cpu().numpy()
        assert S[M] == 5.0
        np.testing.assert_array_equal(S[:M].view(np.uint32), c["s"][kind][:M].view(np.uint32), err_msg="scales")
    return yb, gb


def sweep(torch, pl, c, H, Ms, what, route, start=0):
    """TCSC_GLU_RELU2 on every M, Y type and layout against yardstick (a), Y and dG as whole allocations; the input
    kind and the column scales (set / NULL) rotate so that each M and Y type meets every kind and both settings."""
    n = start
    for M in Ms:
        for ytype in YTYPES:
            for ldy, off in layouts(H):
                kind, cs = KINDS[n % len(KINDS)], (n // 2) % 2 == 0
                tag = f"{what} M={M} {ytype} ldy={ldy} off={off} cs={'set' if cs else 'NULL'} {kind}"
                g, u = gu(c, kind, cs, M)
                yb, gb = run(torch, pl, c, kind, M, H, ldy, off, ytype, cs, "relu2")
                yb.check(ybits(np_relu2(g, u), ytype), tag)
                gb.check(g if route == "mfma" else None, tag)
                n += 1
    return n


# ---- 0. yardstick (b) equals yardstick (a) ----------------------------------------------------------------------------------

def yardstick_b(torch, pl, c, kind, cs, H, M=ROWS):
    """sgemm_i8 twice into fp32 on the kind's quantized rows: the fp32 g and u as tensors."""
    Xq = torch.from_numpy(np.ascontiguousarray(c["q"][kind][:M])).to(DEV)
    Sd = None if c["s"][kind] is None else dev_f32(torch, c["s"][kind][:M])
    out = []
    for plan, b, col in ((pl.gate, c["bg"], c["cg"]), (pl.up, c["bu"], c["cu"])):
        Y = torch.empty((M, H), device=DEV)
        plan.sgemm_i8(Xq, Sd, dev_f32(torch, b), Y, M, H, "basic", 0.0, col_scale=dev_f32(torch, col) if cs else None)
        out.append(Y)
    torch.cuda.synchronize()
    return out


def check_b_equals_a(torch, pl, c, H):
    for kind in KINDS:
        for cs in (True, False):
            gt, ut = yardstick_b(torch, pl, c, kind, cs, H)
            g, u = gu(c, kind, cs)
            for t, a in ((gt, g), (ut, u)):
                np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))
            h = torch.relu(gt).square() * ut
            np.testing.assert_array_equal(h.cpu().numpy().view(np.uint32), np_relu2(g, u).view(np.uint32), err_msg=kind)
            hb = h.to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)
            np.testing.assert_array_equal(hb, np_bf16_bits(np_relu2(g, u)), err_msg=kind)


# ---- 1. the decode route -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("K", KS)
def test_decode_route(gpu, oracle, env, K, H):
    """M <= 16 on packed plans: k_decode8qg where the rule fuses (M = 1, 2, 4 without the norm), the quantizer and
    k_decode8g elsewhere; then everything fused under $TCSC_QFUSE=1 (the norm form too, and M = 5, 16) and nothing
    under $TCSC_QFUSE=0.  dG is never touched."""
    torch = gpu
    c = case(torch, oracle, K, H)
    env()
    pl = Plans(c)
    check_b_equals_a(torch, pl, c, H)
    for M in DECODE_MS:
        for xt in ("f32", "bf16"):
            assert tcsc_amd.launch_info_glu(pl.gate, pl.up, M, xt) == ("decode", 1, M <= 4), (M, xt)
    n = sweep(torch, pl, c, H, DECODE_MS, "decode", "decode")
    env(TCSC_QFUSE="1")
    assert tcsc_amd.launch_info_glu(pl.gate, pl.up, 16, "f32") == ("decode", 1, True)
    n = sweep(torch, pl, c, H, DECODE_MS, "decode QFUSE=1", "decode", start=n + 1)
    env(TCSC_QFUSE="0")
    assert tcsc_amd.launch_info_glu(pl.gate, pl.up, 1, "bf16") == ("decode", 1, False)
    sweep(torch, pl, c, H, (1, 2, 4), "decode QFUSE=0", "decode", start=n + 1)
    pl.free()


# ---- 2. the MFMA route ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("K", KS)
def test_mfma_route(gpu, oracle, env, K, H):
    """M >= 17: k_pack8, k_gemm8w2 into dG and the gated k_gemm8w2; K = 2049 splits by the default rule, so the gated
    k_reduce_i8 runs -- in its 4-column form at H = 16 with an aligned Y of ldy % 4 == 0, in its scalar form
    elsewhere -- and $TCSC_MFMA_WGS=0 gives the unsplit call's bits, which are the same."""
    torch = gpu
    c = case(torch, oracle, K, H)
    env()
    pl = Plans(c)
    for M in GEMM_MS:
        path, slices, fused = tcsc_amd.launch_info_glu(pl.gate, pl.up, M, "f32")
        assert (path, fused) == ("mfma", False) and (slices > 1) == (K == 2049), (M, slices)
    n = sweep(torch, pl, c, H, GEMM_MS, "mfma", "mfma")
    if K == 2049:
        env(TCSC_MFMA_WGS="0")
        assert tcsc_amd.launch_info_glu(pl.gate, pl.up, 33, "f32") == ("mfma", 1, False)
        sweep(torch, pl, c, H, (17, 33), "mfma unsplit", "mfma", start=n + 1)
    pl.free()


@pytest.mark.parametrize("H,vec", [(16, True), (130, False), (260, True)])
def test_a_pinned_split_runs_the_gated_reduce(gpu, oracle, env, H, vec):
    """$TCSC_MFMA_WGS pins two K slices at M = 40, K = 2049 (one tile at H = 16 and 130, two at 260): the gated
    k_reduce_i8 in both forms, against yardstick (a) and so against the unsplit call."""
    torch = gpu
    K, M = 2049, 40
    c = case(torch, oracle, K, H)
    env(TCSC_MFMA_WGS="2" if H < 260 else "4")
    pl = Plans(c)
    assert tcsc_amd.launch_info_glu(pl.gate, pl.up, M, "f32") == ("mfma", 2, False)
    sweep(torch, pl, c, H, (M,), f"pinned split (4-column form where aligned: {vec})", "mfma")
    pl.free()


def test_the_other_kernel_shapes(gpu, oracle, env):
    """The instantiations the small shapes above never reach.  Two column tiles per workgroup on the decode route
    (TG = 2: more than 8 rows and at least 511 column tiles, so that the halved grid still covers 256 CUs), plain,
    fused and fused with the norm; and the 128 x 512 tiles of k_gemm8w2 (at least 128 blocks of 256 x 256: 17 rows by
    32513 columns, K = 16 to keep it small)."""
    torch = gpu
    K, H = 257, 8170  # 511 tiles, the last one ragged
    c = case(torch, oracle, K, H, rows=16)
    env()
    pl = Plans(c, rows=16)
    n = sweep(torch, pl, c, H, (9, 16), "decode TG=2", "decode")
    env(TCSC_QFUSE="1")
    sweep(torch, pl, c, H, (9, 16), "decode TG=2 QFUSE=1", "decode", start=n + 1)
    pl.free()
    env()
    K, H = 16, 32513
    c = case(torch, oracle, K, H, rows=17)
    pl = Plans(c, rows=17)
    assert tcsc_amd.launch_info_glu(pl.gate, pl.up, 17, "f32") == ("mfma", 1, False)
    sweep(torch, pl, c, H, (17,), "mfma 128 x 512 tiles", "mfma")
    pl.free()


# ---- 3. across routes and plan kinds ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,H", [(300, 33), (2049, 130)])
def test_routes_and_plan_kinds_agree(gpu, oracle, env, K, H):
    """M = 16 on the decode route against the first 16 rows of a 17-row call on the MFMA route, both activations and
    both Y types; and ordinary plans with the image against packed plans on either route."""
    torch = gpu
    c = case(torch, oracle, K, H)
    env()
    pl = Plans(c)
    po = Plans(c, packed=False, env=env)
    assert po.ok, "an ordinary plan of 33 columns or more has the images under TCSC_PATH=mfma"
    env()
    for act in ("relu2", "silu"):
        for ytype in YTYPES:
            for kind in ("i8s", "q8b", "q8fn"):
                y16, _ = run(torch, pl, c, kind, 16, H, H, 0, ytype, True, act)
                y17, _ = run(torch, pl, c, kind, 17, H, H, 0, ytype, True, act)
                np.testing.assert_array_equal(y16.values(), y17.values()[:16], err_msg=f"{act} {ytype} {kind}")
                for M, want in ((16, y16), (17, y17)):
                    yo, _ = run(torch, po, c, kind, M, H, H, 0, ytype, True, act)
                    np.testing.assert_array_equal(yo.values(), want.values(), err_msg=f"ordinary {act} {ytype} {kind} {M}")
    pl.free()
    po.free()


def check_silu(h, g, u, rel, what):
    """h (float64 view of the result) against fp64 on the fp32 g and u.  The contract's own formula has a domain: for
    g < -log(FLT_MAX) = -88.7228.. expf(-g) is +inf in fp32, fl(1 + inf) = inf and g / inf = -0, so h is a zero where
    the real value is below 2^-120 |u|; there the test asserts the zero (h == 0), and the relative bound from
    -88.72 up.  In the 0.01 between, where a 1-ulp expf may or may not overflow, either is accepted."""
    g64, u64 = g.astype(np.float64), u.astype(np.float64)
    with np.errstate(over="ignore"):
        h64 = g64 / (1.0 + np.exp(-g64)) * u64
    zero, rel_dom = g64 <= -88.73, g64 >= -88.72
    assert np.all(h[zero] == 0), f"{what}: a nonzero result where expf(-g) overflows"
    ok = np.abs(h - h64) <= rel * np.abs(h64) + 2.0 ** -126
    worst = float(np.max(np.abs(h - h64)[rel_dom] / (np.abs(h64)[rel_dom] + 2.0 ** -126), initial=0.0))
    print(f"{what}: worst relative error {worst:.3g} (bound {rel:.3g}); {int(zero.sum())} of {h.size} in the zero domain")
    assert np.all(ok[rel_dom]), f"{what}: worst relative error {worst:.3g} > {rel:.3g}"
    assert np.all(ok | (h == 0) | zero | rel_dom)
    return worst


# ---- 4. TCSC_GLU_SILU -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,H", [(257, 17), (2049, 130), (300, 16)])
def test_silu(gpu, oracle, env, K, H):
    """The same bits on every route -- decode fused, decode unfused, MFMA, MFMA split / unsplit -- and the derived
    bound against fp64 on the fp32 g and u of yardstick (b)."""
    torch = gpu
    c = case(torch, oracle, K, H)
    env()
    pl = Plans(c)
    kind, cs = "q8b", True
    gt, ut = yardstick_b(torch, pl, c, kind, cs, H)
    g32, u32 = gt.cpu().numpy(), ut.cpu().numpy()

    def fp32_y(M, **knobs):
        env(**knobs)
        yb, _ = run(torch, pl, c, kind, M, H, H, 0, "f32", cs, "silu")
        return yb.values()

    ref = fp32_y(ROWS)  # MFMA, split at K = 2049
    check_silu(ref.view(np.float32).astype(np.float64), g32, u32, SILU_REL, f"silu K={K} H={H}")
    assert np.count_nonzero((g32 < 0) & (g32 > -80)) and np.count_nonzero(g32 > 0)
    np.testing.assert_array_equal(fp32_y(ROWS, TCSC_MFMA_WGS="0"), ref, err_msg="unsplit")
    np.testing.assert_array_equal(fp32_y(17), ref[:17], err_msg="MFMA, 17 rows")
    for M in (1, 4, 16):
        np.testing.assert_array_equal(fp32_y(M, TCSC_QFUSE="1"), ref[:M], err_msg=f"decode fused M={M}")
        np.testing.assert_array_equal(fp32_y(M, TCSC_QFUSE="0"), ref[:M], err_msg=f"decode unfused M={M}")
    env()
    for M in (4, 40):  # a bf16 Y is the rounding of the fp32 one
        yb, _ = run(torch, pl, c, kind, M, H, H + 1, 1, "bf16", cs, "silu")
        yb.check(np_bf16_bits(ref[:M].view(np.float32)), f"silu bf16 M={M}")
    pl.free()


# ---- 5. refusals that need plans, capture, the layers --------------------------------------------------------------------------

def test_refusals_on_live_plans(gpu, oracle, env):
    torch = gpu
    env()
    c, d = case(torch, oracle, 300, 33), case(torch, oracle, 300, 17)
    pl, other = Plans(c), Plans(d)
    Wn = tcsc_amd.TcscMatrix.from_dense(c["Wg"])
    bare = tcsc_amd.Plan(Wn)  # an ordinary plan without the image
    assert not bare.has_w2
    L, P = tcsc_amd.lib(), 0x1000
    ptr = lambda t: C.c_void_p(t.data_ptr())
    Y, B = torch.full((64, 33), SENT, device=DEV), torch.zeros(33, device=DEV)
    Xq = torch.zeros((64, 300), dtype=torch.int8, device=DEV)

    def i8(gate, up, M=4, G=None, ldy=33, X=Xq, bg=B):
        rc = L.tcsc_gpu_sgemm_i8_glu(gate.handle, up.handle, None if X is None else ptr(X), None, None,
                                     None if bg is None else ptr(bg), None, ptr(B), G, ptr(Y), 0, M, ldy, 0, None)
        return rc, tcsc_amd.last_error()

    for gate, up, word in ((bare, pl.up, "gate plan has no 2-bit image"), (pl.gate, bare, "up plan has no 2-bit image"),
                           (pl.gate, other.up, "cols=17"), (other.gate, pl.up, "cols=33")):
        rc, msg = i8(gate, up)
        assert rc == 1 and "tcsc_gpu_sgemm_i8_glu" in msg and word in msg, msg
    rc, msg = i8(pl.gate, pl.up, M=17)
    assert rc == 1 and "dG" in msg and "MFMA" in msg, msg
    rc, msg = i8(pl.gate, pl.up, ldy=32)
    assert rc == 1 and "ldy" in msg, msg
    for kw in (dict(X=None), dict(bg=None)):
        rc, msg = i8(pl.gate, pl.up, **kw)
        assert rc == 1 and "NULL" in msg, msg
    X = torch.zeros((64, 300), device=DEV)
    S = torch.zeros(64, device=DEV)
    rc = L.tcsc_gpu_sgemm_q8_glu(pl.gate.handle, pl.up.handle, ptr(X), 0, None, 0.0, None, ptr(S), None, ptr(B), None,
                                 ptr(B), None, ptr(Y), 0, 5, 33, 0, None)  # M = 5 is not fused: dXq is needed
    assert rc == 1 and "dXq" in tcsc_amd.last_error()
    rc = L.tcsc_gpu_sgemm_q8_glu(pl.gate.handle, pl.up.handle, ptr(X), 0, None, 0.0, ptr(Xq), ptr(S), None, ptr(B), None,
                                 ptr(B), None, ptr(Y), 0, 17, 33, 0, None)
    assert rc == 1 and "dG" in tcsc_amd.last_error()
    torch.cuda.synchronize()
    assert bool((Y == SENT).all()) and bool((S == 0).all()), "a refused call launched something"
    assert L.tcsc_gpu_sgemm_i8_glu(pl.gate.handle, pl.up.handle, None, None, None, ptr(B), None, ptr(B), None, ptr(Y), 0,
                                   0, 33, 0, None) == 0  # no rows: nothing to do
    bare.destroy()
    Wn.free()
    pl.free()
    other.free()


@pytest.mark.parametrize("M", [4, 16, 40])
def test_capture_and_replay(gpu, oracle, env, M):
    """A gated q8 call (with the norm) captured into a graph after reserve: it allocates nothing and does not
    synchronise; the replay on new inputs gives the bits of the eager call."""
    torch = gpu
    K, H = 2049, 130
    c = case(torch, oracle, K, H)
    env()
    pl = Plans(c)
    X = dev_x(torch, c["X"]["bf16"][:M], "bf16")
    Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
    S, G = torch.empty(M, device=DEV), torch.empty((M, H), device=DEV)
    Y = torch.zeros((M, H), dtype=torch.bfloat16, device=DEV)
    bg, bu, cg, cu = (dev_f32(torch, c[k]) for k in ("bg", "bu", "cg", "cu"))
    gamma = dev_f32(torch, c["gamma"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call = lambda: tcsc_amd.sgemm_q8_glu(pl.gate, pl.up, X, Xq, S, bg, bu, Y, M, H, "relu2", cg, cu, gamma, EPS, G,
                                             stream=side.cuda_stream)
        call()  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    Y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    g, u = gu(c, "q8bn", True, M)
    np.testing.assert_array_equal(Y.view(torch.int16).cpu().numpy().view(np.uint16), np_bf16_bits(np_relu2(g, u)))
    pl.free()


def test_layers(gpu, oracle, env):
    """PackedTernaryGLU against the composition by hand, its state_dict round trip through empty(), and
    PackedTernaryMLP against its two layers called one after the other."""
    torch = gpu
    from tcsc_amd import nn

    env()
    K, H = 300, 130
    c = case(torch, oracle, K, H)
    rng = np.random.default_rng(5)
    for act, norm in (("relu2", True), ("silu", False)):
        glu = nn.PackedTernaryGLU(c["Wg"], c["Wu"], c["bg"], c["bu"], c["cg"], 0.37, act=act,
                                  norm_weight=c["gamma"] if norm else None, norm_eps=EPS if norm else None,
                                  out_dtype=torch.bfloat16)
        glu.reserve(40)
        sd = glu.state_dict()
        assert {"w2_gate", "w2_up", "bias_gate", "bias_up", "weight_scale_gate", "weight_scale_up"} <= set(sd)
        assert ("norm_weight" in sd) == norm
        twin = nn.PackedTernaryGLU.empty(K, H, act=act, norm_eps=EPS if norm else None, out_dtype=torch.bfloat16)
        with pytest.raises(tcsc_amd.TcscError):
            twin(torch.zeros((1, K), device=DEV))
        twin.load_state_dict(sd)
        for M in (3, 40):
            x = dev_x(torch, c["X"]["f32"][:M], "f32")
            y = glu(x)
            assert y.dtype == torch.bfloat16 and y.shape == (M, H)
            assert torch.equal(y, twin(x)), "state_dict round trip"
            # by hand: quantize (norm), sgemm_i8 twice, torch
            gl = nn.PackedTernaryLinear(c["Wg"], c["bg"], weight_scale=c["cg"], norm_weight=c["gamma"] if norm else None,
                                        norm_eps=EPS if norm else None)
            ul = nn.PackedTernaryLinear(c["Wu"], c["bu"], weight_scale=0.37, norm_weight=c["gamma"] if norm else None,
                                        norm_eps=EPS if norm else None)
            g, u = gl(x), ul(x)
            if act == "relu2":
                assert torch.equal(y, (torch.relu(g).square() * u).to(torch.bfloat16))
            else:
                # a bf16 Y: half an ulp of its 8 significant bits (2^-9) on top of the fp32 bound, doubled as that is
                check_silu(y.double().cpu().numpy(), g.cpu().numpy(), u.cpu().numpy(), 2.0 ** -8 + SILU_REL,
                           f"layer silu M={M}")
    # an absent buffer is None and is not saved
    plain = nn.PackedTernaryGLU(c["Wg"], c["Wu"])
    assert plain.weight_scale_gate is None and "weight_scale_gate" not in plain.state_dict()
    fl = nn.PackedTernaryGLU.from_float(rng.standard_normal((K, H)).astype(np.float32),
                                        rng.standard_normal((K, H)).astype(np.float32), out_dtype=torch.bfloat16,
                                        norm_eps=EPS)
    Wd = oracle.ternary((H, 64), 0.67, 77)
    down = nn.PackedTernaryLinear(Wd, None, weight_scale=0.02, norm_weight=nc.gamma_of(H, 9), norm_eps=EPS)
    mlp = nn.PackedTernaryMLP(fl, down)
    mlp.reserve(20)
    x = dev_x(torch, c["X"]["bf16"][:20], "bf16")
    y = mlp(x)
    assert y.shape == (20, 64) and y.dtype == torch.float32
    assert torch.equal(y, down(fl(x)))
    with pytest.raises(tcsc_amd.TcscError):
        nn.PackedTernaryMLP(fl, nn.PackedTernaryLinear(c["Wg"]))
