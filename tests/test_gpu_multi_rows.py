"""Gated and grouped int8 calls at 17 .. 64 rows in one decode launch: tcsc_gpu_sgemm_i8_glu /
_q8_glu on k_decode8gr and tcsc_gpu_sgemm_i8_group / _q8_group on k_decode8mr, taken where every plan's
tcsc_gpu_plan_set_decode_rows_multi setting admits M.

The contract is an equality of bits, and the yardsticks are those of tests/test_gpu_decode_rows.py, restated here,
neither of them the new launch itself:
  (a) numpy: the exact integer sums (every |S| asserted below 2^24, so fp64 holds them) through the float32 formula
      v = fl(fl(fl(float32(S)) * s) * c) + b), for the gated call h = fl(fl(r r) u) with r = g < 0 ? 0 : g (i8_glu's
      relu^2), and the rounding to bf16 restated on the bits;
  (b) the same call on the same plans with the setting at 16: k_pack8 and one k_gemm8w2 per matrix.
Every case first asserts the route: launch_info_glu / launch_info_group name `decode` (one slice, not fused) with the
setting on and `mfma` with it off.  Y is compared as integer bits over its whole sentinel-filled allocation, rows
beyond M included.  SiLU has no exact numpy restatement (expf): it is compared bit for bit with (b) and against fp64
with DESIGN §24's bound, |h - h64| <= 5 2^-23 |h64| + 2^-126.

X is full-range int8; in every 16-row tile one row is all -128 and two carry a run of 127, and so does the last live
row of each M.  Shapes are the smallest at which the kernels can go wrong: K around the 16-byte fragment, the 256-k
block and the 8 waves' round, columns around the 16-column tile, and the widths at which the launchers pick each
(row tiles, column tiles) pair on the chip's CU count."""
import numpy as np
import pytest

import tcsc_amd

pytestmark = pytest.mark.gpu

KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")
MS = (17, 32, 33, 48, 49, 64)
KS = (1, 17, 255, 256, 257, 2049, 2304)
GLU_PAIRS = {(2, 2), (2, 1), (4, 1)}  # (row tiles, TG) of DESIGN.md §28
GROUP_PAIRS = {(2, 4), (2, 2), (2, 1), (4, 2), (4, 1)}  # (row tiles, T)
SENT = 7.0
DEV = "cuda:0"
ROWS = 64
AUTO = -1
SILU_REL = 5.0 * 2.0 ** -23
EPS = 1e-5


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    lib = tcsc_amd.lib()
    for name in ("tcsc_gpu_plan_set_decode_rows_multi", "tcsc_gpu_launch_info_glu_decode",
                 "tcsc_gpu_launch_info_group_decode"):  # without the feature: fails here
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


def ybits(v, ytype):
    return np_bf16_bits(v) if ytype == "bf16" else np.ascontiguousarray(v, np.float32).view(np.uint32)


def np_quantize(x):
    x = np.ascontiguousarray(x, np.float32)
    amax = np.max(np.abs(x), axis=1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        live = (amax > 0) & ~np.isinf(np.float32(127.0) / amax)
        scale = np.where(live, amax / np.float32(127.0), np.float32(0)).astype(np.float32)
        inv = np.where(live, np.float32(127.0) / amax, np.float32(0)).astype(np.float32)
    r = np.rint((x * inv[:, None]).astype(np.float32))
    return np.clip(r, -127, 127).astype(np.int8), scale


def check_silu(h, g, u, what):
    """h (the fp32 result) against fp64 on the fp32 g and u, §24's bound.  For g < -log(FLT_MAX) = -88.72.. expf(-g)
    is +inf in fp32 and the contract's own formula gives a zero; in the 0.01 around it either is accepted."""
    h, g64, u64 = h.astype(np.float64), g.astype(np.float64), u.astype(np.float64)
    with np.errstate(over="ignore"):
        h64 = g64 / (1.0 + np.exp(-g64)) * u64
    zero, rel_dom = g64 <= -88.73, g64 >= -88.72
    assert np.all(h[zero] == 0), f"{what}: a nonzero result where expf(-g) overflows"
    ok = np.abs(h - h64) <= SILU_REL * np.abs(h64) + 2.0 ** -126
    worst = float(np.max(np.abs(h - h64)[rel_dom] / (np.abs(h64)[rel_dom] + 2.0 ** -126), initial=0.0))
    print(f"{what}: worst relative error {worst:.3g} (bound {SILU_REL:.3g})")
    assert np.all(ok[rel_dom]), f"{what}: worst relative error {worst:.3g} > {SILU_REL:.3g}"
    assert np.all(ok | (h == 0) | zero | rel_dom)


_cases = {}


def case(o, K, cols):
    """One W per entry of cols (densities 0.67, 0.6, 0.5, 0.75), 64 full-range int8 rows (in every 16-row tile: row 2
    all -128, rows 0 and 15 with a run of 127), per matrix an integer and a float bias and column scales, and
    power-of-two and float row scales -- computed once per shape and left unchanged."""
    key = (K, tuple(cols))
    if key not in _cases:
        seed = 28000 + 3 * K + 5 * sum(cols) + 7 * len(cols)
        rng = np.random.default_rng(seed)
        Xq = rng.integers(-128, 128, (ROWS, K), dtype=np.int64).astype(np.int8)
        for t in range(ROWS // 16):
            Xq[16 * t + 2, :] = -128
            Xq[16 * t, : K // 2 + 1] = 127
            Xq[16 * t + 15, K // 3:] = 127
        pool = np.array([1.0, 0.5, 0.0123, -1.75, 0.0, 3.0, 0.3, -0.0625], np.float32)
        c = dict(K=K, cols=list(cols), Xq=Xq, Wd=[], Bi=[], Bf=[], Cs=[], rows={},
                 s2=np.float32(2.0) ** rng.integers(-6, 4, ROWS).astype(np.float32),
                 sf=(np.abs(o.uniform((ROWS,), seed + 4)) * np.float32(0.05) + np.float32(1e-3)).astype(np.float32))
        for i, N in enumerate(cols):
            c["Wd"].append(o.ternary((K, N), (0.67, 0.6, 0.5, 0.75)[i], seed + 10 * i))
            c["Bi"].append(o.integers((N,), seed + 10 * i + 2))
            c["Bf"].append(o.uniform((N,), seed + 10 * i + 3))
            Cs = pool[rng.integers(0, pool.size, N)]
            Cs[:min(N, 5)] = np.roll(pool, i)[:min(N, 5)]
            c["Cs"].append(Cs.astype(np.float32))
        _cases[key] = c
    return _cases[key]


def rows_of(c, M):
    """(X, [S_i]) of a call of M rows: the case's first M rows with a run of 127 in the last live one, and their sums."""
    if M not in c["rows"]:
        X = c["Xq"][:M].copy()
        X[M - 1, : c["K"] // 3 + 1] = 127
        c["rows"][M] = (X, [int_sums(X, Wd) for Wd in c["Wd"]])
    return c["rows"][M]


# ---- device buffers and plans -------------------------------------------------------------------------------------------

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
    """A sentinel-filled allocation of M + 3 rows of pitch ldy; outputs are column ranges [off, off + N) of it."""

    def __init__(self, torch, M, ldy, ytype):
        self.torch, self.M, self.ldy, self.ytype = torch, M, ldy, ytype
        dt = torch.float32 if ytype == "f32" else torch.bfloat16
        self.Y = torch.full((M + 3, ldy), SENT, dtype=dt, device=DEV)

    def view(self, off, N):
        return self.Y[:, off:off + N]

    def bits(self):
        self.torch.cuda.synchronize()
        if self.ytype == "f32":
            return self.Y.cpu().numpy().view(np.uint32)
        return self.Y.view(self.torch.int16).cpu().numpy().view(np.uint16)

    def check(self, parts, what):
        """parts: [(off, bits of an M x N block)]; everything else must still hold the sentinel."""
        sent = np.float32(SENT).view(np.uint32)
        got = self.bits()
        want = np.full((self.M + 3, self.ldy), sent if self.ytype == "f32" else sent >> 16, got.dtype)
        for off, b in parts:
            want[:self.M, off:off + b.shape[1]] = b
        bad = np.argwhere(got != want)
        if bad.size:
            r, col = bad[0]
            raise AssertionError(f"{what}: {len(bad)} elements differ, the first at row {r} column {col} (M={self.M} "
                                 f"ldy={self.ldy}): got {int(got[r, col]):#x}, expected {int(want[r, col]):#x}")
        return got


class Plans:
    """Packed plans of a case's matrices, every workspace reserved for the MFMA route of 64 rows."""

    def __init__(self, c, reserve=ROWS):
        self.W = [tcsc_amd.TcscMatrix.from_dense(Wd) for Wd in c["Wd"]]
        self.p = [tcsc_amd.Plan.packed(W) for W in self.W]
        for p in self.p:
            assert p.decode_rows_multi == 16
            p.reserve(reserve)

    def set(self, rows):
        for p in self.p:
            p.set_decode_rows_multi(rows)
            assert p.decode_rows_multi == rows

    def free(self):
        for p in self.p:
            p.destroy()
        for W in self.W:
            W.free()


def cus_of(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the gated call -------------------------------------------------------------------------------------------------------

def glu_route(pl, M, want):
    for xt in ("f32", "bf16"):
        info = tcsc_amd.launch_info_glu(pl.p[0], pl.p[1], M, xt)
        if want == "decode":
            assert info == ("decode", 1, False), (M, info)
        else:
            assert info[0] == "mfma" and info[2] is False, (M, info)


def glu_run(torch, pl, c, M, X, s, cs, b, ytype, act, ldy, G):
    H = c["cols"][0]
    yb = YBuf(torch, M, ldy, ytype)
    sv = None if s is None else c[s][:M]
    tcsc_amd.sgemm_i8_glu(pl.p[0], pl.p[1], X, dev_f32(torch, sv), dev_f32(torch, c[b][0]), dev_f32(torch, c[b][1]),
                          yb.view(0, H), M, ldy, act, dev_f32(torch, c["Cs"][0]) if cs else None,
                          dev_f32(torch, c["Cs"][1]) if cs else None, G)
    return yb


def glu_both(torch, pl, c, M, what, s="sf", cs=False, b="Bf", X=None, ytype="f32", act="relu2", ldy=None):
    """The gated call of M rows on the row-tiled launch (G = NULL) and with the setting at 16, both against (a) for
    relu^2; SiLU: the two against each other and, for an fp32 Y, against fp64.  Returns (row tiles, TG)."""
    H = c["cols"][0]
    ldy = ldy or H
    Xm, S = rows_of(c, M)
    Xd = dev_i8(torch, Xm) if X is None else X
    sv = None if s is None else c[s][:M]
    g = np_i8_out(S[0], sv, c["Cs"][0] if cs else None, c[b][0])
    u = np_i8_out(S[1], sv, c["Cs"][1] if cs else None, c[b][1])
    pl.set(64)
    glu_route(pl, M, "decode")
    rt, tg, wgs = tcsc_amd.launch_info_glu_decode(pl.p[0], pl.p[1], M)
    assert rt == (2 if M <= 32 else 4) and rt * 2 * tg <= 8 and wgs == ((H + 15) // 16 + tg - 1) // tg
    yd = glu_run(torch, pl, c, M, Xd, s, cs, b, ytype, act, ldy, None)
    pl.set(16)
    glu_route(pl, M, "mfma")
    ym = glu_run(torch, pl, c, M, Xd, s, cs, b, ytype, act, ldy, torch.empty((M, H), device=DEV))
    if act == "relu2":
        want = ybits(np_relu2(g, u), ytype)
        yd.check([(0, want)], f"{what} M={M}: decode")
        ym.check([(0, want)], f"{what} M={M}: setting 16")
    else:
        ref = ym.bits()[:M, :H].copy()
        got = yd.check([(0, ref)], f"{what} M={M}: silu, decode against the MFMA route")
        if ytype == "f32":
            check_silu(got[:M, :H].view(np.float32), g, u, f"{what} M={M} silu")
    return rt, tg


@pytest.mark.parametrize("K", KS)
def test_glu_rows_and_k(gpu, oracle, env, K):
    """Every M at tile edges with one live row in the last tile, over K around the fragment, the block and the waves'
    round (2049, 2304: wave 0 takes two blocks, the prefetch wraps); K % 16 != 0 takes the byte loads."""
    torch = gpu
    env()
    c = case(oracle, K, (17, 17))
    pl = Plans(c)
    for M in MS:
        glu_both(torch, pl, c, M, f"glu K={K}")
    pl.set(64)
    glu_route(pl, 65, "mfma")
    assert tcsc_amd.launch_info_glu(pl.p[0], pl.p[1], 16)[0] == "decode"
    pl.free()


@pytest.mark.parametrize("H", [1, 17, 130])
def test_glu_columns_and_bits(gpu, oracle, env, H):
    """Columns around the tile; NULL, power-of-two and float row scales, integer and float biases (the integer forms
    are exact in fp32), column scales on both halves, bf16 Y, a pitch; SiLU bit for bit against the MFMA route and
    within §24's bound of fp64."""
    torch = gpu
    env()
    c = case(oracle, 333, (H, H))
    pl = Plans(c)
    for M in (17, 40, 64):
        glu_both(torch, pl, c, M, f"H={H} s=NULL", s=None, b="Bi")
        glu_both(torch, pl, c, M, f"H={H} s=2^e", s="s2", b="Bi", cs=True)
        glu_both(torch, pl, c, M, f"H={H} float", cs=True)
        glu_both(torch, pl, c, M, f"H={H} bf16", cs=True, ytype="bf16", ldy=H + 3)
        glu_both(torch, pl, c, M, f"H={H} pitch", ldy=H + 5)
        glu_both(torch, pl, c, M, f"H={H}", act="silu", cs=True)
        glu_both(torch, pl, c, M, f"H={H} bf16", act="silu", ytype="bf16", s="s2")
    pl.free()


def test_glu_g_is_untouched_on_the_decode_route(gpu, oracle, env):
    torch = gpu
    env()
    c = case(oracle, 257, (40, 40))
    pl = Plans(c)
    M, H = 40, 40
    Xm, S = rows_of(c, M)
    pl.set(64)
    glu_route(pl, M, "decode")
    G = torch.full((M + 1, H), SENT, device=DEV)
    yb = glu_run(torch, pl, c, M, dev_i8(torch, Xm), "sf", True, "Bf", "f32", "relu2", H, G)
    g = np_i8_out(S[0], c["sf"][:M], c["Cs"][0], c["Bf"][0])
    u = np_i8_out(S[1], c["sf"][:M], c["Cs"][1], c["Bf"][1])
    yb.check([(0, ybits(np_relu2(g, u), "f32"))], "decode with a G buffer")
    assert np.all(G.cpu().numpy().view(np.uint32) == np.float32(SENT).view(np.uint32)), "dG was written"
    pl.set(16)
    with pytest.raises(tcsc_amd.TcscError, match="NULL dG on the MFMA route"):  # a raw pointer: nothing allocates one
        tcsc_amd.sgemm_i8_glu(pl.p[0], pl.p[1], dev_i8(torch, Xm).data_ptr(), None, dev_f32(torch, c["Bf"][0]),
                              dev_f32(torch, c["Bf"][1]), yb.Y.data_ptr(), M, H, "relu2", ytype="f32")
    pl.free()


def test_glu_every_instantiation(gpu, oracle, env):
    """The widths at which launch_info_glu_decode reports each (row tiles, TG) pair on this chip, TG = 2 with a ragged
    last workgroup; at each pair both load forms (X aligned, X one byte off) and both Y types.  The pairs seen are
    exactly DESIGN's."""
    torch = gpu
    env()
    cus = cus_of(torch)
    K = 272
    seen = set()
    for H in (130, 16 * (2 * cus + 1) - 8):
        c = case(oracle, K, (H, H))
        pl = Plans(c)
        tiles = (H + 15) // 16
        for M in (24, 40):
            rt, tg, wgs = tcsc_amd.launch_info_glu_decode(pl.p[0], pl.p[1], M)
            assert tg == 1 or (tiles % tg != 0 and wgs >= cus), "a ragged last workgroup on a grid that covers the chip"
            seen.add((rt, tg))
            Xm, _ = rows_of(c, M)
            for offset in (0, 1):
                Xd = dev_i8(torch, Xm, offset)
                for ytype in ("f32", "bf16"):
                    assert glu_both(torch, pl, c, M, f"H={H} {ytype} off={offset}", X=Xd, ytype=ytype, cs=True) == (rt, tg)
        pl.free()
    assert seen == GLU_PAIRS, seen


# ---- the grouped call -----------------------------------------------------------------------------------------------------

def group_route(pl, M, want):
    n = len(pl.p)
    for xt in ("f32", "bf16"):
        info = tcsc_amd.launch_info_group(pl.p, M, xt)
        if want == "decode":
            assert info == ("decode", [1] * n, False), (M, info)
        else:
            assert info[0] == "mfma" and info[2] is False, (M, info)


def group_layout(cols, fused):
    """Column offsets and the pitch of the members' outputs: slices of one tensor at odd element offsets with sentinel
    columns between and behind them (fused), or each at its own offset 0 of its own tensor of pitch N + 2."""
    if not fused:
        return None, None
    offs, at = [], 1
    for N in cols:
        offs.append(at)
        at += N + 2 - N % 2  # the next offset is odd again
    return offs, at + 3


def group_run(torch, pl, c, M, X, s, cs, b, ytype, fused):
    cols, n = c["cols"], len(c["cols"])
    sv = None if s is None else c[s][:M]
    offs, pitch = group_layout(cols, fused)
    if fused:
        bufs = [YBuf(torch, M, pitch, ytype)] * n
        Ys = [bufs[0].view(offs[i], cols[i]) for i in range(n)]
    else:
        bufs = [YBuf(torch, M, N + 2, ytype) for N in cols]
        offs = [0] * n
        Ys = [bufs[i].view(0, cols[i]) for i in range(n)]
    tcsc_amd.sgemm_i8_group(pl.p, X, dev_f32(torch, sv), [dev_f32(torch, v) for v in c[b]], Ys, M,
                            col_scales=[dev_f32(torch, v) if cs else None for v in c["Cs"]])
    return bufs, offs


def group_check(bufs, offs, want, what):
    if all(bf is bufs[0] for bf in bufs):
        bufs[0].check(list(zip(offs, want)), what)
    else:
        for i, bf in enumerate(bufs):
            bf.check([(offs[i], want[i])], f"{what}, member {i}")


def group_both(torch, pl, c, M, what, s="sf", cs=False, b="Bf", X=None, ytype="f32", fused=True):
    """The grouped call of M rows on the row-tiled launch and with the setting at 16, both against (a).  Returns
    (row tiles, T)."""
    cols = c["cols"]
    Xm, S = rows_of(c, M)
    Xd = dev_i8(torch, Xm) if X is None else X
    sv = None if s is None else c[s][:M]
    want = [ybits(np_i8_out(S[i], sv, c["Cs"][i] if cs else None, c[b][i]), ytype) for i in range(len(cols))]
    pl.set(64)
    group_route(pl, M, "decode")
    rt, t, wgs = tcsc_amd.launch_info_group_decode(pl.p, M)
    assert rt == (2 if M <= 32 else 4) and rt * t <= 8 and wgs == sum(((N + 15) // 16 + t - 1) // t for N in cols)
    group_check(*group_run(torch, pl, c, M, Xd, s, cs, b, ytype, fused), want, f"{what} M={M}: decode")
    pl.set(16)
    group_route(pl, M, "mfma")
    group_check(*group_run(torch, pl, c, M, Xd, s, cs, b, ytype, fused), want, f"{what} M={M}: setting 16")
    return rt, t


@pytest.mark.parametrize("K", KS)
def test_group_rows_and_k(gpu, oracle, env, K):
    torch = gpu
    env()
    c = case(oracle, K, (17, 1))
    pl = Plans(c)
    for M in MS:
        group_both(torch, pl, c, M, f"group K={K}")
    pl.set(64)
    group_route(pl, 65, "mfma")
    assert tcsc_amd.launch_info_group(pl.p, 16)[0] == "decode"
    pl.free()


@pytest.mark.parametrize("cols", [(130,), (130, 17, 1), (1, 130, 17, 33)])
def test_group_counts_and_bits(gpu, oracle, env, cols):
    """Counts 1, 3 and 4 with ragged column counts; outputs as slices of one fused tensor at odd element offsets and in
    tensors of their own with sentinel columns; NULL, power-of-two and float row scales; column scales; bf16.  Each
    member equals its own sgemm_i8 with col_scale on its own plan, bit for bit."""
    torch = gpu
    env()
    c = case(oracle, 333, cols)
    pl = Plans(c)
    for M in (17, 40, 64):
        group_both(torch, pl, c, M, f"{cols} s=NULL", s=None, b="Bi")
        group_both(torch, pl, c, M, f"{cols} s=2^e", s="s2", b="Bi", cs=True, fused=False)
        group_both(torch, pl, c, M, f"{cols} float", cs=True)
        group_both(torch, pl, c, M, f"{cols} bf16", cs=True, ytype="bf16")
        group_both(torch, pl, c, M, f"{cols} bf16 own tensors", ytype="bf16", fused=False)
        # the members' own calls
        Xm, _ = rows_of(c, M)
        Xd, Sd = dev_i8(torch, Xm), dev_f32(torch, c["sf"][:M])
        pl.set(64)
        group_route(pl, M, "decode")
        for ytype in ("f32", "bf16"):
            bufs, offs = group_run(torch, pl, c, M, Xd, "sf", True, "Bf", ytype, True)
            got = bufs[0].bits()
            for i, N in enumerate(cols):
                own = YBuf(torch, M, N, ytype)
                pl.p[i].sgemm_i8(Xd, Sd, dev_f32(torch, c["Bf"][i]), own.Y, M, N, "basic", 0.0,
                                 col_scale=dev_f32(torch, c["Cs"][i]))
                np.testing.assert_array_equal(got[:M, offs[i]:offs[i] + N], own.bits()[:M], err_msg=f"member {i} {ytype}")
    pl.free()


def test_group_every_instantiation(gpu, oracle, env):
    """The widths at which launch_info_group_decode reports each (row tiles, T) pair on this chip, every member with a
    ragged last workgroup where T > 1 and a ragged last tile; at each pair both load forms and both Y types.  The
    pairs seen are exactly DESIGN's."""
    torch = gpu
    env()
    cus = cus_of(torch)
    K = 272
    seen = set()
    for cols in ((130, 17, 1), (16 * (cus + 1) - 8,) * 2, (16 * (2 * cus + 1) - 8,) * 2):
        c = case(oracle, K, cols)
        pl = Plans(c)
        for M in (24, 40):
            rt, t, wgs = tcsc_amd.launch_info_group_decode(pl.p, M)
            assert t == 1 or (all(((N + 15) // 16) % t for N in cols) and wgs >= cus), "ragged, and the grid covers the chip"
            seen.add((rt, t))
            Xm, _ = rows_of(c, M)
            for offset in (0, 1):
                Xd = dev_i8(torch, Xm, offset)
                for ytype in ("f32", "bf16"):
                    assert group_both(torch, pl, c, M, f"{cols} {ytype} off={offset}", X=Xd, ytype=ytype, cs=True) == (rt, t)
        pl.free()
    assert seen == GROUP_PAIRS, seen


# ---- routing ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("qfuse", [None, "1"])
def test_q8_forms_are_the_quantizer_then_these_kernels(gpu, oracle, env, qfuse):
    """sgemm_q8_glu and sgemm_q8_group at M = 40, fp32 and bf16 x, with and without the norm: decode, never fused
    (whatever $TCSC_QFUSE says), the bits and row scales of the same call with the setting at 16 -- and, without the
    norm, of the numpy quantizer and formula."""
    torch = gpu
    K, M = 333, 40
    cg = case(oracle, K, (77, 77))
    cm = case(oracle, K, (130, 17, 1))
    env(TCSC_QFUSE=qfuse)
    pg, pm = Plans(cg), Plans(cm)
    rng = np.random.default_rng(2840)
    X32 = (rng.standard_normal((M, K)) * rng.choice([1e-3, 1.0, 37.0], (M, 1))).astype(np.float32)
    X32[2] = 0.0
    gamma = dev_f32(torch, 1.0 + 0.1 * rng.standard_normal(K))
    for xt in ("f32", "bf16"):
        X = dev_f32(torch, X32) if xt == "f32" else dev_f32(torch, X32).to(torch.bfloat16)
        q, s = np_quantize(X.to(torch.float32).cpu().numpy())
        want_g = ybits(np_relu2(np_i8_out(int_sums(q, cg["Wd"][0]), s, cg["Cs"][0], cg["Bf"][0]),
                                np_i8_out(int_sums(q, cg["Wd"][1]), s, cg["Cs"][1], cg["Bf"][1])), "bf16")
        want_m = [ybits(np_i8_out(int_sums(q, cm["Wd"][i]), s, cm["Cs"][i], cm["Bf"][i]), "bf16") for i in range(3)]
        offs, pitch = group_layout(cm["cols"], True)
        got = {}
        for rows in (64, 16):
            pg.set(rows), pm.set(rows)
            glu_route(pg, M, "decode" if rows == 64 else "mfma")
            group_route(pm, M, "decode" if rows == 64 else "mfma")
            for norm in (False, True):
                nw, ne = (gamma, EPS) if norm else (None, None)
                yg = YBuf(torch, M, 80, "bf16")
                Xq = torch.zeros((M, K), dtype=torch.int8, device=DEV)
                Sc = torch.full((M + 1,), 5.0, device=DEV)
                G = None if rows == 64 else torch.empty((M, 77), device=DEV)
                tcsc_amd.sgemm_q8_glu(pg.p[0], pg.p[1], X, Xq, Sc, dev_f32(torch, cg["Bf"][0]), dev_f32(torch, cg["Bf"][1]),
                                      yg.view(0, 77), M, 80, "relu2", dev_f32(torch, cg["Cs"][0]),
                                      dev_f32(torch, cg["Cs"][1]), nw, ne, G)
                ym = YBuf(torch, M, pitch, "bf16")
                Xq2 = torch.zeros((M, K), dtype=torch.int8, device=DEV)
                Sc2 = torch.full((M + 1,), 5.0, device=DEV)
                tcsc_amd.sgemm_q8_group(pm.p, X, Xq2, Sc2, [dev_f32(torch, v) for v in cm["Bf"]],
                                        [ym.view(offs[i], cm["cols"][i]) for i in range(3)], M,
                                        col_scales=[dev_f32(torch, v) for v in cm["Cs"]], norm_weight=nw, norm_eps=ne)
                if not norm:
                    yg.check([(0, want_g)], f"q8 glu {xt} rows={rows}")
                    ym.check(list(zip(offs, want_m)), f"q8 group {xt} rows={rows}")
                    for t in (Xq, Xq2):  # unfused: the quantizer wrote its scratch
                        np.testing.assert_array_equal(t.cpu().numpy(), q)
                got[rows, norm] = [yg.bits().copy(), ym.bits().copy(), Sc.cpu().numpy(), Sc2.cpu().numpy()]
                assert got[rows, norm][2][M] == 5.0 and got[rows, norm][3][M] == 5.0
        for norm in (False, True):
            for a, b in zip(got[64, norm], got[16, norm]):
                np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                              b.view(np.uint32) if b.dtype == np.float32 else b, err_msg=f"{xt} norm={norm}")
        # the decode route needs dXq above 16 rows, whatever $TCSC_QFUSE says
        pg.set(64), pm.set(64)
        with pytest.raises(tcsc_amd.TcscError, match="NULL dXq"):
            tcsc_amd.sgemm_q8_glu(pg.p[0], pg.p[1], X, None, Sc, dev_f32(torch, cg["Bf"][0]), dev_f32(torch, cg["Bf"][1]),
                                  yg.view(0, 77), M, 80, "relu2")
        with pytest.raises(tcsc_amd.TcscError, match="NULL dXq"):
            tcsc_amd.sgemm_q8_group(pm.p, X, None, Sc2, [dev_f32(torch, v) for v in cm["Bf"]],
                                    [ym.view(offs[i], cm["cols"][i]) for i in range(3)], M)
    pg.free(), pm.free()


def test_mixed_settings_and_the_setter(gpu, oracle, env):
    """The call decodes only when every plan admits M: one plan at 16, or one at AUTO (which asks the call's own rule),
    keeps it on the MFMA route; set_decode_rows (§27's setting) is not read; the setter's refusals."""
    torch = gpu
    env()
    cus = cus_of(torch)
    K, M = 65, 40
    c = case(oracle, K, (130, 17, 1))
    pl = Plans(c)
    glu = Plans(case(oracle, K, (40, 40)))
    # §27's setting alone changes nothing here
    for p in pl.p + glu.p:
        p.set_decode_rows(64)
    group_route(pl, M, "mfma"), glu_route(glu, M, "mfma")
    # a number admits M <= rows
    pl.set(40), glu.set(40)
    for m, want in ((16, "decode"), (17, "decode"), (40, "decode"), (41, "mfma"), (64, "mfma"), (65, "mfma")):
        assert tcsc_amd.launch_info_group(pl.p, m)[0] == want and tcsc_amd.launch_info_glu(*glu.p, m)[0] == want, m
    # one plan at 16
    for k in range(3):
        pl.set(64)
        pl.p[k].set_decode_rows_multi(16)
        group_route(pl, M, "mfma")
        if k:  # the members before it, alone, still decode
            assert tcsc_amd.launch_info_group(pl.p[:k], M)[0] == "decode"
    for k in range(2):
        glu.set(64)
        glu.p[k].set_decode_rows_multi(16)
        glu_route(glu, M, "mfma")
    # one plan at AUTO: the call's own rule decides, per call
    gpays = tcsc_amd.group_rows_pays(M, K, c["cols"], cus)
    hpays = tcsc_amd.glu_rows_pays(M, K, 40, cus)
    pl.set(64), glu.set(64)
    pl.p[1].set_decode_rows_multi(AUTO)
    glu.p[0].set_decode_rows_multi(AUTO)
    assert pl.p[1].decode_rows_multi == AUTO
    group_route(pl, M, "decode" if gpays else "mfma")
    glu_route(glu, M, "decode" if hpays else "mfma")
    pl.set(AUTO), glu.set(AUTO)
    for m in (1, 16, 17, 32, 33, 64, 65):
        want_g = "decode" if m <= 16 or tcsc_amd.group_rows_pays(m, K, c["cols"], cus) else "mfma"
        want_h = "decode" if m <= 16 or tcsc_amd.glu_rows_pays(m, K, 40, cus) else "mfma"
        assert tcsc_amd.launch_info_group(pl.p, m)[0] == want_g and tcsc_amd.launch_info_glu(*glu.p, m)[0] == want_h, m
    # the bits under a mixed setting are the call's
    pl.set(64)
    pl.p[2].set_decode_rows_multi(16)
    Xm, S = rows_of(c, M)
    want = [ybits(np_i8_out(S[i], c["sf"][:M], None, c["Bf"][i]), "f32") for i in range(3)]
    group_check(*group_run(torch, pl, c, M, dev_i8(torch, Xm), "sf", False, "Bf", "f32", True), want, "mixed")
    # refusals
    p = pl.p[0]
    p.set_decode_rows_multi(40)
    for rows in (15, 65, 0, -2, 1 << 20):
        with pytest.raises(tcsc_amd.TcscError, match="tcsc_gpu_plan_set_decode_rows_multi"):
            p.set_decode_rows_multi(rows)
        assert p.decode_rows_multi == 40
    assert p.decode_rows == 64  # the two settings do not touch each other
    for m in (0, 65):
        with pytest.raises(tcsc_amd.TcscError, match="tcsc_gpu_launch_info_group_decode"):
            tcsc_amd.launch_info_group_decode(pl.p, m)
        with pytest.raises(tcsc_amd.TcscError, match="tcsc_gpu_launch_info_glu_decode"):
            tcsc_amd.launch_info_glu_decode(*glu.p, m)
    assert [tcsc_amd.launch_info_group_decode(pl.p, m)[0] for m in (16, 17, 33)] == [1, 2, 4]
    assert [tcsc_amd.launch_info_glu_decode(*glu.p, m)[0] for m in (16, 17, 33)] == [1, 2, 4]
    pl.free(), glu.free()
    # a plan without the image
    env(TCSC_PATH="mfma")
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"][0])
    plain = tcsc_amd.Plan(W)
    plain.reserve(17)
    assert plain.enable_i8() and not plain.has_w2
    with pytest.raises(tcsc_amd.TcscError, match="2-bit image"):
        plain.set_decode_rows_multi(64)
    assert plain.decode_rows_multi == 16
    plain.destroy()
    W.free()


# ---- capture --------------------------------------------------------------------------------------------------------------

def test_captured_calls_replay_on_new_inputs(gpu, oracle, env):
    """A captured gated call and a captured grouped call of 40 rows on plans that reserved nothing: each replayed
    twice on new inputs; no plan's memory grows."""
    torch = gpu
    env()
    K, M = 1000, 40
    cg = case(oracle, K, (300, 300))
    cm = case(oracle, K, (130, 17, 1))
    pg, pm = Plans(cg, reserve=1), Plans(cm, reserve=1)
    pg.set(64), pm.set(64)
    glu_route(pg, M, "decode"), group_route(pm, M, "decode")
    held = [p.info()["device_bytes"] for p in pg.p + pm.p]
    side = torch.cuda.Stream()
    Qg = torch.zeros((M, K), dtype=torch.int8, device=DEV)
    Sg = torch.zeros(M, device=DEV)
    Yg = torch.empty((M, 300), device=DEV)
    Ym = torch.empty((M, 148), device=DEV)
    Ys = list(torch.split(Ym, [130, 17, 1], dim=1))
    Bg = [dev_f32(torch, v) for v in cg["Bf"]]
    Bm = [dev_f32(torch, v) for v in cm["Bf"]]
    torch.cuda.synchronize()
    gg, gm = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gg, stream=side):
        tcsc_amd.sgemm_i8_glu(pg.p[0], pg.p[1], Qg, Sg, Bg[0], Bg[1], Yg, M, 300, "relu2", G=None,
                              stream=torch.cuda.current_stream().cuda_stream)
    with torch.cuda.graph(gm, stream=side):
        tcsc_amd.sgemm_i8_group(pm.p, Qg, Sg, Bm, Ys, M, stream=torch.cuda.current_stream().cuda_stream)
    assert [p.info()["device_bytes"] for p in pg.p + pm.p] == held
    for first in (0, 24):
        X = cg["Xq"][first:first + M]
        sv = cg["sf"][first:first + M]
        Qg.copy_(dev_i8(torch, X))
        Sg.copy_(dev_f32(torch, sv))
        Yg.fill_(float("nan")), Ym.fill_(float("nan"))
        torch.cuda.synchronize()
        gg.replay(), gm.replay()
        torch.cuda.synchronize()
        want = np_relu2(np_i8_out(int_sums(X, cg["Wd"][0]), sv, None, cg["Bf"][0]),
                        np_i8_out(int_sums(X, cg["Wd"][1]), sv, None, cg["Bf"][1]))
        np.testing.assert_array_equal(Yg.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=f"glu from row {first}")
        wm = np.concatenate([np_i8_out(int_sums(X, cm["Wd"][i]), sv, None, cm["Bf"][i]) for i in range(3)], axis=1)
        np.testing.assert_array_equal(Ym.cpu().numpy().view(np.uint32), wm.view(np.uint32), err_msg=f"group from row {first}")
        assert [p.info()["device_bytes"] for p in pg.p + pm.p] == held
    del gg, gm
    pg.free(), pm.free()


# ---- the layers -------------------------------------------------------------------------------------------------------------

def test_the_layers(gpu, oracle, env):
    """PackedTernaryGLU.set_decode_rows(64) and PackedTernaryGroup.set_decode_rows(64) at M = 40 match the layers at
    the default setting bit for bit; a loaded state dict builds plans that carry the setting."""
    torch = gpu
    env()
    from tcsc_amd.nn import PackedTernaryGLU, PackedTernaryGroup

    K, M = 300, 40
    cg = case(oracle, K, (130, 130))
    cm = case(oracle, K, (130, 17, 1))
    x = dev_f32(torch, oracle.uniform((M, K), 28501))
    gamma = 1.0 + 0.1 * np.random.default_rng(28).standard_normal(K).astype(np.float32)

    def glu():
        return PackedTernaryGLU(cg["Wd"][0], cg["Wd"][1], cg["Bf"][0], cg["Bf"][1], 0.37, 0.21, "relu2", gamma, EPS,
                                torch.bfloat16)

    def group():
        return PackedTernaryGroup(cm["Wd"], cm["Bf"], [0.37, 0.21, 1.5], gamma, EPS)

    base_g, on_g, base_m, on_m = glu(), glu(), group(), group()
    on_g.set_decode_rows(64), on_m.set_decode_rows(64)
    assert [p.decode_rows_multi for p in base_g.plans + base_m.plans] == [16] * 5
    assert [p.decode_rows_multi for p in on_g.plans + on_m.plans] == [64] * 5
    assert tcsc_amd.launch_info_glu(*base_g.plans, M)[0] == "mfma" and tcsc_amd.launch_info_glu(*on_g.plans, M)[0] == "decode"
    assert tcsc_amd.launch_info_group(base_m.plans, M)[0] == "mfma" and tcsc_amd.launch_info_group(on_m.plans, M)[0] == "decode"
    with torch.no_grad():
        y0, y1 = base_g(x), on_g(x)
        m0, m1 = base_m(x), on_m(x)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y1.view(torch.int16).cpu().numpy(), y0.view(torch.int16).cpu().numpy())
    for a, b in zip(m0, m1):
        np.testing.assert_array_equal(b.contiguous().cpu().numpy().view(np.uint32), a.contiguous().cpu().numpy().view(np.uint32))
    empty = PackedTernaryGroup.empty(K, [130, 17, 1], norm_eps=EPS)
    empty.set_decode_rows(64)
    empty.load_state_dict(base_m.state_dict())
    assert [p.decode_rows_multi for p in empty.plans] == [64] * 3
    with torch.no_grad():
        m2 = empty(x)
    torch.cuda.synchronize()
    for a, b in zip(m0, m2):
        np.testing.assert_array_equal(b.contiguous().cpu().numpy().view(np.uint32), a.contiguous().cpu().numpy().view(np.uint32))
