"""tcsc_gpu_sgemm_i8_group / tcsc_gpu_sgemm_q8_group: up to four matrices on one X in one call, on
every kernel that finishes one: k_decode8m at T = 1, 2 and 4, k_decode8qm, and k_gemm8w2 / k_reduce_i8 once per
member on one packed X.

The contract is an equality of bits of every member's Y against two yardsticks, neither of them the code under test:
  (a) numpy: the quantizer (and the norm) restated in float32, the exact integer sums, and the epilogue
      fl(fl(fl(float(S) s) c) + b) with the bf16 rounding restated on the bits (tests/test_gpu_out.py, norm_cases.py);
  (b) the existing entry point: Plan.sgemm_i8 per member on the quantized rows, asserted equal to (a) once per case
      on all its rows, so every grouped result that equals (a) equals (b).
Every Y is compared as its whole sentinel-filled allocation (the YBuf of tests/test_gpu_out.py), in two layouts: each
member in a tensor of its own (the pitches and offsets of test_gpu_out.layouts), and all members as column slices of
one tensor at odd element offsets with a common pitch and a spare column between neighbours."""
import ctypes as C

import numpy as np
import pytest

import norm_cases as nc
import tcsc_amd
from test_gpu_out import DEV, KNOBS, SENT, YBuf, col_scales, dev_f32, dev_x, formula, int_sums, layouts, np_quantize
from test_gpu_out import ordinary_plan

pytestmark = pytest.mark.gpu

KS = (16, 257, 300, 2049)
COLS = ((33, 16, 17), (1, 1), (130,), (15, 260, 16, 1))
DECODE_MS = (1, 2, 4, 5, 16)
GEMM_MS = (17, 33, 130)
ROWS = 130
YTYPES = ("f32", "bf16")
KINDS = ("i8s", "i8n", "q8f", "q8b", "q8fn", "q8bn")  # int8 X with / without row scales; fp32 / bf16 X; with the norm
EPS = 1e-5


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

_cases = {}


def case(torch, o, K, cols, rows=ROWS):
    """The members' W, `rows` rows of X, and per input kind the numpy quantization (after the numpy norm where the kind
    has one) with the exact sums against every member; a bias and column scales per member.  Computed once per shape
    and left unchanged; a test of M rows uses the first M."""
    key = (K, tuple(cols), rows)
    if key in _cases:
        return _cases[key]
    seed = 25000 + 3 * K + 5 * sum(cols) + len(cols)
    rng = np.random.default_rng(seed)
    c = dict(cols=tuple(cols), W=[o.ternary((K, n), (0.67, 0.6, 0.5, 0.75)[i], seed + i) for i, n in enumerate(cols)])
    X = (rng.standard_normal((rows, K)) * rng.choice([1e-2, 1.0, 37.0], (rows, 1))).astype(np.float32)
    X[2 % rows] = 0.0  # a row of zeros: scale 0, Y = b
    Xb = torch.from_numpy(X).to(torch.bfloat16).to(torch.float32).numpy()
    c["gamma"] = nc.gamma_of(K, seed + 7)
    c["X"] = {"f32": X, "bf16": Xb}
    c["b"] = [o.uniform((n,), seed + 10 + i) for i, n in enumerate(cols)]
    c["cs"] = [col_scales(n, seed + 20 + i) for i, n in enumerate(cols)]
    c["q"], c["s"], c["S"] = {}, {}, {}
    for kind in KINDS:
        if kind.startswith("i8"):
            q, s = np_quantize(X)
            if kind == "i8n":
                s = None
            else:
                s = (s * np.float32(0.75)).astype(np.float32)  # fixed scales of the caller's, not the quantizer's
        else:
            x = c["X"]["bf16" if kind[2] == "b" else "f32"]
            if kind.endswith("n"):
                x = nc.np_rmsnorm(x, c["gamma"], EPS)[0]
            q, s = np_quantize(x)
        c["q"][kind], c["s"][kind] = q, s
        c["S"][kind] = [int_sums(q, W) for W in c["W"]]
    _cases[key] = c
    return c


def want_bits(c, kind, cs, ytype, M):
    """Yardstick (a): the bits of every member's Y on the first M rows."""
    s = None if c["s"][kind] is None else c["s"][kind][:M]
    return [formula(c["S"][kind][i][:M], s, c["cs"][i] if cs else None, c["b"][i], "basic", ytype)
            for i in range(len(c["cols"]))]


# ---- the plans and the calls ----------------------------------------------------------------------------------------------

class Plans:
    def __init__(self, c, packed=True, env=None, reserve=ROWS):
        self.W, self.p = [], []
        for Wd in c["W"]:
            if packed:
                W = tcsc_amd.TcscMatrix.from_dense(Wd)
                p = tcsc_amd.Plan.packed(W)
                if reserve:
                    p.reserve(reserve)
            else:
                W, p = ordinary_plan(env, Wd, reserve)
            self.W.append(W)
            self.p.append(p)

    ok = property(lambda self: all(p is not None for p in self.p))

    def free(self):
        for p in self.p:
            if p is not None:
                p.destroy()
        for W in self.W:
            W.free()


def sent_bits(ytype):
    s = np.float32(SENT).view(np.uint32)
    return s if ytype == "f32" else np.uint16(s >> 16)


class Outs:
    """The outputs of one grouped call.  own: a YBuf per member, the layouts of test_gpu_out rotating with n.  Otherwise
    one YBuf of which member i is the column slice from starts[i] on: the base is one element into the allocation and
    every start is even, so every member's first element sits at an odd element offset, and between neighbours there
    is at least one spare column that must keep the sentinel."""

    def __init__(self, torch, M, cols, ytype, own, n=0):
        self.own, self.cols, self.M, self.ytype = own, cols, M, ytype
        if own:
            lay = [layouts(N)[(n + i) % 5] for i, N in enumerate(cols)]
            self.bufs = [YBuf(torch, M, N, ldy, off, ytype) for N, (ldy, off) in zip(cols, lay)]
            self.Ys, self.ldys = [b.Y for b in self.bufs], [ldy for ldy, _ in lay]
            return
        self.starts, at = [], 0
        for N in cols:
            self.starts.append(at)
            at += N + 1
            at += at & 1
        self.width = self.starts[-1] + cols[-1]
        ldy = self.width + 1 + n % 3
        self.big = YBuf(torch, M, self.width, ldy, 1, ytype)
        self.Ys, self.ldys = [self.big.Y[s:] for s in self.starts], [ldy] * len(cols)
        assert all((1 + s) % 2 == 1 for s in self.starts)

    def check(self, bits, what):
        if self.own:
            for i, (b, w) in enumerate(zip(self.bufs, bits)):
                b.check(w, f"{what} member {i}")
            return
        full = np.full((self.M, self.width), sent_bits(self.ytype), bits[0].dtype)
        for s, N, w in zip(self.starts, self.cols, bits):
            full[:, s:s + N] = w
        self.big.check(full, what + " (slices of one tensor)")

    def untouched(self):
        return all(b.untouched() for b in (self.bufs if self.own else [self.big]))

    def values(self):
        if self.own:
            return [b.values() for b in self.bufs]
        v = self.big.values()
        return [v[:, s:s + N] for s, N in zip(self.starts, self.cols)]


def run(torch, plans, c, kind, M, ytype, cs, own=True, n=0, Xq_scratch=True):
    """One grouped call on the first M rows into fresh sentinel-filled outputs.  The scales a q8 call writes are checked
    against the numpy quantizer's here."""
    out = Outs(torch, M, c["cols"], ytype, own, n)
    bs = [dev_f32(torch, b) for b in c["b"]]
    cols = [dev_f32(torch, x) for x in c["cs"]] if cs else None
    if kind.startswith("i8"):
        Xq = torch.from_numpy(np.ascontiguousarray(c["q"][kind][:M])).to(DEV)
        Sd = None if c["s"][kind] is None else dev_f32(torch, c["s"][kind][:M])
        tcsc_amd.sgemm_i8_group(plans, Xq, Sd, bs, out.Ys, M, out.ldys, cols)
    else:
        xt = "bf16" if kind[2] == "b" else "f32"
        X = dev_x(torch, c["X"][xt][:M], xt)
        Xq = torch.empty((M, X.shape[1]), dtype=torch.int8, device=DEV) if Xq_scratch else None
        S = torch.full((M + 1,), 5.0, device=DEV)
        norm = kind.endswith("n")
        tcsc_amd.sgemm_q8_group(plans, X, Xq, S, bs, out.Ys, M, out.ldys, cols,
                                dev_f32(torch, c["gamma"]) if norm else None, EPS if norm else None)
        torch.cuda.synchronize()
        S = S.cpu().numpy()
        assert S[M] == 5.0
        np.testing.assert_array_equal(S[:M].view(np.uint32), c["s"][kind][:M].view(np.uint32), err_msg="scales")
    return out


def sweep(torch, plans, c, Ms, what, start=0):
    """Every M, Y type and layout against yardstick (a), every Y as its whole allocation; the input kind and the column
    scales (set / NULL) rotate so that each M and Y type meets every kind and both settings."""
    n = start
    for M in Ms:
        for ytype in YTYPES:
            for own in (True, False):
                kind, cs = KINDS[n % len(KINDS)], (n // 2) % 2 == 0
                tag = f"{what} M={M} {ytype} own={own} cs={'set' if cs else 'NULL'} {kind}"
                run(torch, plans, c, kind, M, ytype, cs, own, n).check(want_bits(c, kind, cs, ytype, M), tag)
                n += 1
    return n


def check_b_equals_a(torch, pl, c, rows=ROWS):
    """Yardstick (b), Plan.sgemm_i8 per member on the quantized rows, equals yardstick (a): once per case."""
    for kind in KINDS:
        Xq = torch.from_numpy(np.ascontiguousarray(c["q"][kind][:rows])).to(DEV)
        Sd = None if c["s"][kind] is None else dev_f32(torch, c["s"][kind][:rows])
        for cs in (True, False):
            for ytype in YTYPES:
                want = want_bits(c, kind, cs, ytype, rows)
                for i, (plan, N) in enumerate(zip(pl.p, c["cols"])):
                    yb = YBuf(torch, rows, N, N, 0, ytype)
                    plan.sgemm_i8(Xq, Sd, dev_f32(torch, c["b"][i]), yb.Y, rows, N, "basic", 0.0,
                                  col_scale=dev_f32(torch, c["cs"][i]) if cs else None)
                    yb.check(want[i], f"yardstick (b) {kind} member {i}")


# ---- 1. the decode route -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", COLS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("K", KS)
def test_decode_route(gpu, oracle, env, K, cols):
    """M <= 16 on packed plans: k_decode8qm where the rule fuses (M = 1, 2, 4 without the norm), the quantizer and
    k_decode8m elsewhere; then under $TCSC_QFUSE=1 (everything without the norm fused, M = 5 and 16 too) and under
    $TCSC_QFUSE=0 (nothing).  With the norm the call is never fused, whatever launch_info_group reports for the call
    without it, and the bits are the same."""
    torch = gpu
    c = case(torch, oracle, K, cols)
    env()
    pl = Plans(c)
    check_b_equals_a(torch, pl, c)
    ones = [1] * len(cols)
    for M in DECODE_MS:
        for xt in ("f32", "bf16"):
            assert tcsc_amd.launch_info_group(pl.p, M, xt) == ("decode", ones, M <= 4), (M, xt)
    n = sweep(torch, pl.p, c, DECODE_MS, "decode")
    env(TCSC_QFUSE="1")
    for M in DECODE_MS:
        assert tcsc_amd.launch_info_group(pl.p, M, "f32") == ("decode", ones, True)
    n = sweep(torch, pl.p, c, DECODE_MS, "decode QFUSE=1", start=n + 1)
    env(TCSC_QFUSE="0")
    for M in DECODE_MS:
        assert tcsc_amd.launch_info_group(pl.p, M, "bf16") == ("decode", ones, False)
    sweep(torch, pl.p, c, (1, 2, 4), "decode QFUSE=0", start=n + 1)
    pl.free()


# ---- 2. T = 2 and T = 4 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols,Ms,T", [((4090, 33, 4090), (5, 8), 2), ((8170, 17, 8200), (9, 16), 4)])
def test_two_and_four_tiles_per_workgroup(gpu, oracle, env, cols, Ms, T):
    """The instantiations small shapes never reach on 256 CUs: 258 workgroups at T = 2 (256, 3 and 256 column tiles)
    and at T = 4 (511, 2 and 513 tiles: a one-block member in the middle, ragged last tiles and last blocks), plain
    and with everything fused under $TCSC_QFUSE=1."""
    torch = gpu
    K = 257
    assert sum(((n + 15) // 16 + T - 1) // T for n in cols) == 258
    c = case(torch, oracle, K, cols, rows=16)
    env()
    pl = Plans(c, reserve=0)
    check_b_equals_a(torch, pl, c, rows=16)
    assert tcsc_amd.launch_info_group(pl.p, Ms[0], "f32") == ("decode", [1, 1, 1], False)
    n = sweep(torch, pl.p, c, Ms, f"decode T={T}")
    env(TCSC_QFUSE="1")
    assert tcsc_amd.launch_info_group(pl.p, Ms[1], "bf16") == ("decode", [1, 1, 1], True)
    sweep(torch, pl.p, c, Ms, f"decode T={T} QFUSE=1", start=n + 1)
    pl.free()


# ---- 3. the MFMA route ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", COLS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("K", KS)
def test_mfma_route(gpu, oracle, env, K, cols):
    """M >= 17: the quantizer once, k_pack8 once, k_gemm8w2 per member with its slabs in its own workspace.  K = 2049
    splits by the default rule (k_reduce_i8 per member), and $TCSC_MFMA_WGS=0 gives the same bits unsplit."""
    torch = gpu
    c = case(torch, oracle, K, cols)
    env()
    pl = Plans(c)
    for M in GEMM_MS:
        path, slices, fused = tcsc_amd.launch_info_group(pl.p, M, "f32")
        assert (path, fused, len(slices)) == ("mfma", False, len(cols))
        assert all((s > 1) == (K == 2049) for s in slices), (M, slices)
    n = sweep(torch, pl.p, c, GEMM_MS, "mfma")
    if K == 2049:
        env(TCSC_MFMA_WGS="0")
        assert tcsc_amd.launch_info_group(pl.p, 33, "f32") == ("mfma", [1] * len(cols), False)
        sweep(torch, pl.p, c, (17, 33), "mfma unsplit", start=n + 1)
    pl.free()


def test_mfma_workspaces(gpu, oracle, env):
    """Members reserved to different max_M (the second too small for the call: it is grown first) and members with
    nothing reserved (all grown on first use) give the bits of the reserved call."""
    torch = gpu
    K, cols = 2049, (33, 16, 17)
    c = case(torch, oracle, K, cols)
    env()
    for reserve in ((130, 17, 64), (0, 0, 0)):
        pl = Plans(c, reserve=0)
        for p, r in zip(pl.p, reserve):
            if r:
                p.reserve(r)
        n = 0
        for M in (130, 40):
            for kind in ("q8bn", "i8s"):
                run(torch, pl.p, c, kind, M, "bf16", True, n % 2 == 0, n).check(want_bits(c, kind, True, "bf16", M),
                                                                              f"reserve={reserve} M={M} {kind}")
                n += 1
        pl.free()


# ---- 4. across routes and plan kinds ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,cols", [(300, (33, 130, 40)), (2049, (130, 33))])
def test_routes_and_plan_kinds_agree(gpu, oracle, env, K, cols):
    """M = 16 on the decode route against the first 16 rows of a 17-row call on the MFMA route; ordinary plans with the
    image (tcsc_gpu_plan_enable_w2) against packed plans on either route."""
    torch = gpu
    c = case(torch, oracle, K, cols)
    env()
    pl = Plans(c)
    po = Plans(c, packed=False, env=env)
    assert po.ok, "an ordinary plan of 33 columns or more has the images under TCSC_PATH=mfma"
    env()
    for ytype in YTYPES:
        for kind in ("i8s", "q8b", "q8fn"):
            y16 = run(torch, pl.p, c, kind, 16, ytype, True).values()
            y17 = run(torch, pl.p, c, kind, 17, ytype, True, own=False).values()
            for a, b in zip(y16, y17):
                np.testing.assert_array_equal(a, b[:16], err_msg=f"{ytype} {kind}")
            for M, want in ((16, y16), (17, y17)):
                yo = run(torch, po.p, c, kind, M, ytype, True).values()
                for i, (a, b) in enumerate(zip(yo, want)):
                    np.testing.assert_array_equal(a, b, err_msg=f"ordinary {ytype} {kind} M={M} member {i}")
    pl.free()
    po.free()


@pytest.mark.parametrize("K,N", [(300, 130), (2049, 33)])
def test_a_group_of_one_is_the_single_call(gpu, oracle, env, K, N):
    """One member: the bits of Plan.sgemm_i8 / Plan.sgemm_q8_norm on that plan, into the same layout, on both routes,
    and launch_info_group's fused is launch_info_q8's."""
    torch = gpu
    c = case(torch, oracle, K, (N,))
    env()
    pl = Plans(c)
    plan, n = pl.p[0], 0
    b, cs, gamma = dev_f32(torch, c["b"][0]), dev_f32(torch, c["cs"][0]), dev_f32(torch, c["gamma"])
    for M in (1, 4, 5, 16, 17, 40):
        assert tcsc_amd.launch_info_group([plan], M, "bf16")[2] == plan.launch_info_q8(M, "bf16")[2]
        for ytype in YTYPES:
            ldy, off = layouts(N)[n % 5]
            n += 1
            Xq = torch.from_numpy(np.ascontiguousarray(c["q"]["i8s"][:M])).to(DEV)
            Sd = dev_f32(torch, c["s"]["i8s"][:M])
            single, group = YBuf(torch, M, N, ldy, off, ytype), YBuf(torch, M, N, ldy, off, ytype)
            plan.sgemm_i8(Xq, Sd, b, single.Y, M, ldy, "basic", 0.0, col_scale=cs)
            tcsc_amd.sgemm_i8_group([plan], Xq, Sd, [b], [group.Y], M, [ldy], [cs])
            np.testing.assert_array_equal(group.bits(), single.bits(), err_msg=f"i8 M={M} {ytype}")
            X = dev_x(torch, c["X"]["bf16"][:M], "bf16")
            Xs = torch.empty((M, K), dtype=torch.int8, device=DEV)
            S1, S2 = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
            single, group = YBuf(torch, M, N, ldy, off, ytype), YBuf(torch, M, N, ldy, off, ytype)
            plan.sgemm_q8_norm(X, Xs, S1, b, single.Y, M, ldy, gamma, EPS, "basic", 0.0, col_scale=cs)
            tcsc_amd.sgemm_q8_group([plan], X, Xs, S2, [b], [group.Y], M, [ldy], [cs], gamma, EPS)
            np.testing.assert_array_equal(group.bits(), single.bits(), err_msg=f"q8 norm M={M} {ytype}")
            assert torch.equal(S1, S2)
            single.check(want_bits(c, "q8bn", True, ytype, M)[0], f"single q8 norm M={M} {ytype}")
    pl.free()


# ---- 5. refusals that need plans, capture, the layer ---------------------------------------------------------------------------

def test_refusals_on_live_plans(gpu, oracle, env):
    """A member without the image, members of different K, ldy < cols and a NULL dXq where the call is not fused: each
    names the call and the member's index, and launches nothing."""
    torch = gpu
    env()
    c, d = case(torch, oracle, 300, (33, 16, 17)), case(torch, oracle, 257, (130,))
    pl, other = Plans(c), Plans(d)
    Wn = tcsc_amd.TcscMatrix.from_dense(c["W"][1])
    bare = tcsc_amd.Plan(Wn)  # an ordinary plan without the image
    assert not bare.has_w2
    L = tcsc_amd.lib()
    cols = c["cols"]
    bs = [torch.zeros(n, device=DEV) for n in cols]
    Xq = torch.zeros((64, 300), dtype=torch.int8, device=DEV)
    X, S = torch.zeros((64, 300), device=DEV), torch.zeros(64, device=DEV)
    out = Outs(torch, 16, cols, "f32", True)

    def refused(word, index, plans=pl.p, ldys=None, M=4, q8=False, Xq_=Xq, **kw):
        with pytest.raises(tcsc_amd.TcscError) as e:
            if q8:
                tcsc_amd.sgemm_q8_group(plans, X, Xq_, S, bs, out.Ys, M, ldys or out.ldys, **kw)
            else:
                tcsc_amd.sgemm_i8_group(plans, Xq_, None, bs, out.Ys, M, ldys or out.ldys)
        msg = tcsc_amd.last_error()
        name = "tcsc_gpu_sgemm_q8_group" if q8 else "tcsc_gpu_sgemm_i8_group"
        assert name in msg and word in msg and (index is None or f"member {index}" in msg), msg
        assert name in str(e.value)

    for q8 in (False, True):
        refused("2-bit image", 1, plans=[pl.p[0], bare, pl.p[2]], q8=q8)
        refused("K=257", 2, plans=[pl.p[0], pl.p[1], other.p[0]], q8=q8)
        refused("ldy=15", 1, ldys=[out.ldys[0], 15, out.ldys[2]], q8=q8)
    refused("dXq", None, M=5, q8=True, Xq_=None)  # M = 5 is not fused by the rule
    refused("dXq", None, M=2, q8=True, Xq_=None, norm_eps=EPS)  # with the norm nothing is
    with pytest.raises(tcsc_amd.TcscError, match="member 1"):
        tcsc_amd.launch_info_group([pl.p[0], bare], 4)
    # the C entry point itself: the return code and the message
    arr, n = tcsc_amd._group_members([pl.p[0], bare], bs[:2], out.Ys[:2], out.ldys[:2])
    assert L.tcsc_gpu_sgemm_i8_group(arr, n, C.c_void_p(Xq.data_ptr()), None, 0, 4, None) == 1
    assert "member 1" in L.tcsc_gpu_last_error().decode()
    torch.cuda.synchronize()
    assert out.untouched() and bool((S == 0).all()), "a refused call launched something"
    # no rows: nothing to do, whatever X is
    tcsc_amd.sgemm_i8_group(pl.p, None, None, bs, out.Ys, 0, out.ldys)
    tcsc_amd.sgemm_q8_group(pl.p, None, None, None, bs, out.Ys, 0, out.ldys, xtype="f32")
    assert out.untouched()
    # a fused call needs no dXq
    env(TCSC_QFUSE="1")
    run(torch, pl.p, c, "q8b", 16, "f32", True, Xq_scratch=False).check(want_bits(c, "q8b", True, "f32", 16), "no dXq")
    bare.destroy()
    Wn.free()
    pl.free()
    other.free()


@pytest.mark.parametrize("M", [4, 16, 40])
def test_capture_and_replay(gpu, oracle, env, M):
    """A grouped q8 call (with the norm, into column slices of one bf16 tensor) captured into a graph after reserve: it
    allocates nothing and does not synchronise; the replay gives the bits of the eager call and of yardstick (a)."""
    torch = gpu
    K, cols = 2049, (33, 16, 17)
    c = case(torch, oracle, K, cols)
    env()
    pl = Plans(c, reserve=M)
    X = dev_x(torch, c["X"]["bf16"][:M], "bf16")
    Xq = torch.empty((M, K), dtype=torch.int8, device=DEV)
    S = torch.empty(M, device=DEV)
    Y = torch.zeros((M, sum(cols)), dtype=torch.bfloat16, device=DEV)
    Ys = list(torch.split(Y, list(cols), dim=1))
    bs, cs = [dev_f32(torch, b) for b in c["b"]], [dev_f32(torch, x) for x in c["cs"]]
    gamma = dev_f32(torch, c["gamma"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call = lambda: tcsc_amd.sgemm_q8_group(pl.p, X, Xq, S, bs, Ys, M, None, cs, gamma, EPS, stream=side.cuda_stream)
        call()  # the eager call, outside the capture
        side.synchronize()
        eager = Y.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    Y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Y.view(torch.int16), eager.view(torch.int16))
    want = np.concatenate(want_bits(c, "q8bn", True, "bf16", M), axis=1)
    np.testing.assert_array_equal(Y.view(torch.int16).cpu().numpy().view(np.uint16), want)
    pl.free()


def test_layer(gpu, oracle, env):
    """PackedTernaryGroup.from_float on three matrices with a norm against three PackedTernaryLinear layers built from
    the same inputs, bit for bit at 1, 16 and 40 rows; the state_dict round trip through empty(); the outputs are views
    of one allocation."""
    torch = gpu
    from tcsc_amd import nn

    env()
    K, cols = 300, (130, 33, 40)
    rng = np.random.default_rng(25)
    Wf = [rng.standard_normal((K, n)).astype(np.float32) for n in cols]
    bs = [rng.standard_normal(n).astype(np.float32) for n in cols]
    gamma = nc.gamma_of(K, 26)
    x40 = (rng.standard_normal((40, K)) * 3).astype(np.float32)
    for dt in (torch.bfloat16, torch.float32):
        grp = nn.PackedTernaryGroup.from_float(Wf, bs, norm_weight=gamma, norm_eps=EPS, out_dtype=dt)
        grp.reserve(40)
        singles = [nn.PackedTernaryLinear.from_float(W, b, norm_weight=gamma, norm_eps=EPS, out_dtype=dt)
                   for W, b in zip(Wf, bs)]
        sd = grp.state_dict()
        assert {f"{k}_{i}" for k in ("w2", "bias", "weight_scale") for i in range(3)} | {"norm_weight"} <= set(sd)
        twin = nn.PackedTernaryGroup.empty(K, cols, norm_eps=EPS, out_dtype=dt)
        with pytest.raises(tcsc_amd.TcscError):
            twin(torch.zeros((1, K), device=DEV))
        twin.load_state_dict(sd)
        for M in (1, 16, 40):
            x = dev_x(torch, x40[:M], "bf16" if dt == torch.bfloat16 else "f32")
            ys = grp(x)
            assert isinstance(ys, tuple) and [tuple(y.shape) for y in ys] == [(M, n) for n in cols]
            base = ys[0].untyped_storage().data_ptr()
            assert all(y.untyped_storage().data_ptr() == base and y.dtype == dt for y in ys), "views of one allocation"
            assert [y.storage_offset() for y in ys] == [0, cols[0], cols[0] + cols[1]]
            assert M == 1 or all(y.stride() == (sum(cols), 1) for y in ys)  # one row: its stride is torch's to choose
            for y, lin, t in zip(ys, singles, twin(x)):
                assert torch.equal(y, lin(x)), f"against PackedTernaryLinear at M={M}"
                assert torch.equal(y, t), "state_dict round trip"
        assert grp(x.reshape(2, 20, K))[1].shape == (2, 20, cols[1]) and grp(x[0])[2].shape == (cols[2],)
    plain = nn.PackedTernaryGroup([oracle.ternary((K, 17), 0.67, 3)])
    assert plain.weight_scale_0 is None and "weight_scale_0" not in plain.state_dict()
    with pytest.raises(tcsc_amd.TcscError):
        nn.PackedTernaryGroup([oracle.ternary((K, 17), 0.67, 3), oracle.ternary((K + 1, 17), 0.67, 4)])
    with pytest.raises(tcsc_amd.TcscError):
        nn.PackedTernaryGroup([oracle.ternary((K, 2), 0.67, i) for i in range(5)])
