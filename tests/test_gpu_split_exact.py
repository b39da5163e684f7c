"""All 24 bits of x through every route of the MFMA path (csrc/tcsc_mfma.hip).

The path splits x into three bf16 parts h + m + l, routes them through k_split3,
the x3_index layout, the LDS-DMA rings and their swizzle, k_gemm3, then
k_reduce_fix or k_fixup / exact_out, and promises the same 24 bits back.  The
integer tests elsewhere draw |x| <= 512 (10 bits: l is always 0, m carries 1-2
bits) and the float tests' bound cannot see a wrong l at one k.  Here every
comparison is bit for bit, with no tolerance:

* the wide-integer probe (tests/test_split_probe.py: every k meets an entry whose
  h, m and l are all nonzero, every sum is an integer below 2^24 times a power of
  two, so exact in fp32 in any order) on every tile shape, split and unsplit, at
  scales 2^-101 (every row flagged: the whole output is exact_out's), 2^-100
  (nothing flagged, the smallest parts at the bottom of the range) and 2^100;
* one nonzero per row over the whole exponent range, where Y[r, j] = W[r, j] * x_r.

Expected outputs come from the oracle's restatement of the reference's loops and
from a float64 product; both must agree with each other and with the GPU.
"""
import numpy as np
import pytest

import pyoracle
import tcsc_amd
from test_gpu_backward import transposed_plan
from test_split_probe import (PROBE_SHAPES, expect_f64, onehot_flagged, onehot_values, onehot_x, probe_case)

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    return tcsc_amd.lib()


@pytest.fixture
def path(monkeypatch):
    """path(mode): TCSC_PATH for plans created from now on, host-API cache dropped, the
    host API in its fast mode (as tests/test_gpu_mfma.py's fixture)."""
    monkeypatch.setenv("TCSC_HOST_FAST", "1")

    def set_mode(mode):
        if mode is None:
            monkeypatch.delenv("TCSC_PATH", raising=False)
        else:
            monkeypatch.setenv("TCSC_PATH", mode)
        tcsc_amd.cache_clear()

    yield set_mode
    monkeypatch.delenv("TCSC_PATH", raising=False)
    monkeypatch.delenv("TCSC_HOST_FAST", raising=False)
    tcsc_amd.cache_clear()


class Launcher:
    """One plan of W[:, c0:c1] and one set of device buffers, launched as often as asked."""

    def __init__(self, W, M, K, c0=0, c1=None, ldy=None):
        import torch

        self.torch, dev = torch, torch.device("cuda:0")
        self.c0, self.c1 = c0, W.cols if c1 is None else c1
        self.nc, self.M = self.c1 - c0, M
        self.ldy = ldy or self.nc
        self.plan = tcsc_amd.Plan(W, c0, self.c1)
        self.dX = torch.empty((M, K), device=dev)
        self.dB = torch.empty((self.nc,), device=dev)
        self.dY = torch.empty((M, self.ldy), device=dev)

    def __call__(self, X, B, variant, a, prepared=False):
        torch = self.torch
        self.dX.copy_(torch.from_numpy(np.array(X, np.float32)))  # copies: the shared inputs are read-only
        self.dB.copy_(torch.from_numpy(np.array(B[self.c0:self.c1], np.float32)))
        self.dY.fill_(SENTINEL)
        if prepared:
            self.plan.prepare_x(self.dX, self.M)
            self.plan.sgemm_prepared(self.dB, self.dY, self.M, self.ldy, variant, a)
        else:
            self.plan.sgemm(self.dX, self.dB, self.dY, self.M, self.ldy, variant, a)
        torch.cuda.synchronize()
        Y = self.dY.cpu().numpy()
        assert np.all(Y[:, self.nc:] == SENTINEL), "columns beyond the plan's were written"
        return Y[:, :self.nc]

    def launch(self):
        return self.plan.launch_info(self.M)

    def info(self):
        return self.plan.info()

    def close(self):
        self.plan.destroy()


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        r, c = np.nonzero(bad)
        raise AssertionError(
            f"{what}: {bad.sum()} of {bad.size} outputs differ, in {np.unique(r).size} rows and "
            f"{np.unique(c).size} columns; first at ({r[0]}, {c[0]}): {got[r[0], c[0]]!r}, expected "
            f"{want[r[0], c[0]]!r} (rows {np.unique(r)[:8]}, columns {np.unique(c)[:8]})")


_cases, _linear, _expect = {}, {}, {}


def case(oracle, name, scale=0):
    """(Wd, X, B, Wref) of a named probe case, made once and never modified."""
    key = (name, scale)
    if key not in _cases:
        Wd, X, B = probe_case(oracle, name, scale)
        for arr in (Wd, X, B):
            arr.setflags(write=False)
        wkey = (name, "W")
        if wkey not in _cases:
            _cases[wkey] = oracle.tcsc_from_dense(Wd)
        _cases[key] = (Wd, X, B, _cases[wkey])
    return _cases[key]


def expected(oracle, name, variant, a, scale=0, oracle_rows=None):
    """The expected output from the float64 product (made once per case and scale), after
    checking that the oracle's loops give the same bits (on `oracle_rows`, default every row)."""
    key = (name, variant, a, scale)
    if key not in _expect:
        Wd, X, B, Wref = case(oracle, name, scale)
        if (name, scale) not in _linear:
            _linear[name, scale] = expect_f64(X, Wd, B)
        v = _linear[name, scale]
        want = np.where(v < 0, np.float32(a) * v, v) if variant in pyoracle.PRELU_VARIANTS else v.copy()
        sub = slice(None) if oracle_rows is None else oracle_rows
        assert_bits(oracle.sgemm(variant, X[sub], Wref, B, a), want[sub], f"oracle vs float64, {name} {variant}")
        want.setflags(write=False)
        _expect[key] = want
    return _expect[key]


def mfma_launcher(path, oracle, name, scale=0, **kw):
    path("mfma")
    Wd, X, B, _ = case(oracle, name, scale)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    return W, Launcher(W, X.shape[0], X.shape[1], **kw)


# ---- 128 x 128 tiles, unsplit ------------------------------------------------

@pytest.mark.parametrize("name,variants", [("unsplit_ragged", pyoracle.VARIANTS),
                                           ("unsplit_k64", ("basic", "prelu_onthego"))])
def test_unsplit_small_tiles(gpu, oracle, path, name, variants):
    """K = 701: a ragged last 64-k block (the zero fill past K, the clamped DMA tail), X's
    scalar loads; K = 704: whole blocks, the 16-B loads."""
    W, run = mfma_launcher(path, oracle, name)
    _, X, B, _ = case(oracle, name)
    for variant in variants:
        Y = run(X, B, variant, 0.2)
        assert run.launch() == ("mfma", 1), run.launch()
        assert_bits(Y, expected(oracle, name, variant, 0.2), f"{name} {variant}")
    run.close()
    W.free()


# ---- split K -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["split_256", "split_100", "split_130"])
def test_split_k_small_tiles(gpu, oracle, path, name):
    W, run = mfma_launcher(path, oracle, name)
    _, X, B, _ = case(oracle, name)
    for variant in pyoracle.VARIANTS:
        Y = run(X, B, variant, 0.2)
        assert run.launch()[0] == "mfma" and run.launch()[1] > 1, run.launch()
        assert_bits(Y, expected(oracle, name, variant, 0.2), f"{name} {variant} {run.launch()}")
    run.close()
    W.free()


@pytest.mark.parametrize("name", ["narrow_64", "narrow_33", "narrow_17"])
def test_narrow_tiles_split_and_unsplit(gpu, oracle, path, monkeypatch, name):
    """M <= 64: the 64 x 256 tiles, K split by the cost model and unsplit ($TCSC_MFMA_WGS=0)."""
    W, run = mfma_launcher(path, oracle, name)
    _, X, B, _ = case(oracle, name)
    for wgs, split in ((None, True), ("0", False)):
        if wgs is None:
            monkeypatch.delenv("TCSC_MFMA_WGS", raising=False)
        else:
            monkeypatch.setenv("TCSC_MFMA_WGS", wgs)
        for variant in ("basic", "prelu_separate"):
            Y = run(X, B, variant, 0.2)
            launch = run.launch()
            assert launch[0] == "mfma" and (launch[1] > 1) == split, launch
            assert_bits(Y, expected(oracle, name, variant, 0.2), f"{name} {variant} {launch}")
    run.close()
    W.free()


# ---- column blocks, pitch, prepared launches -----------------------------------

def test_column_block_pitch_and_prepared(gpu, oracle, path):
    name = "unsplit_ragged"
    Wd, X, B, _ = case(oracle, name)
    path("mfma")
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    want = expected(oracle, name, "prelu_separate", 0.2)
    for c0, c1, ldy in ((3, 270, 271), (100, 229, 140)):
        run = Launcher(W, X.shape[0], X.shape[1], c0=c0, c1=c1, ldy=ldy)
        for prepared in (False, True):
            Y = run(X, B, "prelu_separate", 0.2, prepared=prepared)  # the sentinel columns are checked inside
            assert run.launch() == ("mfma", 1), run.launch()
            assert_bits(Y, np.ascontiguousarray(want[:, c0:c1]), f"[{c0},{c1}) ldy={ldy} prepared={prepared}")
        run.close()
    W.free()


# ---- the backward product on a transposed MFMA plan ----------------------------

def test_sgemm_t_on_a_transposed_mfma_plan(gpu, oracle, monkeypatch):
    import torch

    M, N, K, density, seed = PROBE_SHAPES["transposed"]  # the plan's shape: G is M x N, W^T N x K
    Wd, G, _ = probe_case(oracle, "transposed")           # Wd here is W^T (N x K)
    W = tcsc_amd.TcscMatrix.from_dense(np.ascontiguousarray(Wd.T))  # W: K x N = 512 x 1024
    assert (W.rows, W.cols) == (512, 1024) and M == 256
    plan = transposed_plan(monkeypatch, W, "mfma", M)
    print("transposed plan launch:", plan.launch_info(M))
    dG = torch.from_numpy(G).to("cuda:0")
    dX = torch.full((M, K + 5), SENTINEL, device="cuda:0")
    plan.sgemm_t(dG, dX, M, K + 5, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dX.cpu().numpy()
    zeros = np.zeros(K, np.float32)
    want = expect_f64(G, Wd, zeros)  # G @ (W^T) in float64
    assert_bits(oracle.sgemm("basic", G, oracle.tcsc_from_dense(Wd), zeros), want, "oracle vs float64")
    assert (got[:, K:] == SENTINEL).all()
    assert_bits(np.ascontiguousarray(got[:, :K]), want, "dX")
    plan.destroy()
    W.free()


# ---- the host API's cached plan --------------------------------------------------

def test_host_api_fast_mode_cached_plan(gpu, oracle, path):
    name = "unsplit_ragged"
    W, run = mfma_launcher(path, oracle, name)
    _, X, B, _ = case(oracle, name)
    run(X, B, "basic", 0.2)
    assert run.launch() == ("mfma", 1)  # the host API's plan is created under the same settings
    run.close()
    for variant in ("basic", "prelu_onthego"):
        for call in range(2):  # the second call finds the plan in the cache
            assert_bits(tcsc_amd.sgemm(variant, X, W, B, 0.2), expected(oracle, name, variant, 0.2),
                        f"host {variant} call {call}")
    W.free()


# ---- controls: the same generator on the other kernel families -----------------

@pytest.mark.parametrize("name,want_path", [("gather", "gather"), ("gather_split", "gather"), ("small_m", "small")])
def test_controls_other_paths(gpu, oracle, path, monkeypatch, name, want_path):
    path("gather" if want_path == "gather" else None)
    if want_path == "gather":  # the K split is this case's subject, not the cost model's choice
        monkeypatch.setenv("TCSC_SLICES", "4" if name == "gather_split" else "1")
    Wd, X, B, _ = case(oracle, name)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    run = Launcher(W, X.shape[0], X.shape[1])
    for variant in ("basic", "prelu_onthego"):
        Y = run(X, B, variant, 0.2)
        launch = run.launch()
        assert launch[0] == want_path and (launch[1] > 1) == (name == "gather_split"), launch
        assert_bits(Y, expected(oracle, name, variant, 0.2), f"{name} {variant} {launch}")
    run.close()
    W.free()


# ---- the scale sweep: the flag threshold from both sides, the top of the range -----

@pytest.mark.parametrize("name,slices", [("unsplit_ragged", 1), ("split_100", 4)])
def test_scale_sweep_on_one_plan(gpu, oracle, path, name, slices):
    """2^-100: nothing flagged, the smallest parts are the smallest the GEMM may see.  2^-101:
    every row flagged, so the whole output is exact_out's (k_fixup, or k_reduce_fix where K is
    split).  2^100: sums up to 2^124.  One plan, one set of buffers, each scale after another
    one: the flags are written by every call."""
    W, run = mfma_launcher(path, oracle, name)
    for scale in (-100, -101, -100, 100, -101, 0):
        _, X, B, _ = case(oracle, name, scale)
        for variant in ("basic", "prelu_onthego"):
            Y = run(X, B, variant, 0.5)
            assert run.launch() == ("mfma", slices), run.launch()
            assert_bits(Y, expected(oracle, name, variant, 0.5, scale), f"{name} 2^{scale} {variant}")
    run.close()
    W.free()


# ---- one nonzero per row, over the whole exponent range ----------------------------

@pytest.mark.parametrize("K,N,density,seed,route", [
    (701, 300, 0.5, 1300, ("mfma", 1)),
    (1100, 257, 0.5, 1310, ("mfma", 2)),  # 9 x 3 tiles of 128 x 128, 18 blocks: the model splits them in 2
    (333, 200, 0.05, 1320, ("gather", 1))])
def test_one_hot_rows_whole_exponent_range(gpu, oracle, path, monkeypatch, K, N, density, seed, route):
    """X = diag(x): Y[r, j] = W[r, j] * x_r exactly, whatever the order.  x holds FLT_MAX, 2^-100
    and 2^-100 (1 + 2^-16 + 2^-23) (unflagged: l = 2^-123), and on flagged rows the value just
    below 2^-100, 2^-126, 2^-127 and 2^-149."""
    path(route[0])
    if route[0] == "gather":
        monkeypatch.setenv("TCSC_SLICES", "1")
    x = onehot_values(K, seed)
    X, B = onehot_x(x), np.zeros(N, np.float32)
    Wd = oracle.ternary((K, N), density, seed + 1)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    run = Launcher(W, K, K)
    want = Wd * x[:, None]
    assert want.dtype == np.float32 and np.isfinite(want).all()
    for variant, rows in (("basic", np.arange(K)), ("prelu_basic", np.flatnonzero(np.abs(x) >= 2.0 ** -125))):
        Y = run(X, B, variant, 0.5)
        launch = run.launch()
        print(f"one-hot K={K} N={N} {variant}: {launch}, {int(onehot_flagged(x).sum())} flagged rows")
        assert launch == route, launch
        w = want if variant == "basic" else np.where(want < 0, np.float32(0.5) * want, want)
        assert not np.isnan(Y).any()
        bad = Y[rows] != w[rows]
        if bad.any():
            r = rows[np.nonzero(bad)[0]]
            raise AssertionError(f"{variant} {launch}: {bad.sum()} outputs differ, rows {np.unique(r)[:12]} "
                                 f"(x = {x[np.unique(r)[:12]]!r}, flagged {onehot_flagged(x)[np.unique(r)[:12]]})")
    run.close()
    W.free()


# ---- the 128 x 512 tiles (last: the largest launches) ----------------------------------

def test_big_tiles_ragged_everything(gpu, oracle, path):
    """M = 2050 (a short last band of row tiles, a ragged last tile), N = 4000 (a ragged last
    column tile), K = 333 (a ragged last block).  The whole output against the float64 product;
    the oracle's loops on the rows around every row-tile edge."""
    name = "big_ragged"
    W, run = mfma_launcher(path, oracle, name)
    _, X, B, _ = case(oracle, name)
    M = X.shape[0]
    edge = np.unique(np.clip(np.concatenate([np.arange(0, M, 128) - 1, np.arange(0, M, 128), [M - 1]]), 0, M - 1))
    for variant in ("basic", "prelu_basic"):
        Y = run(X, B, variant, 0.2)
        assert run.info()["mfma_min_M"] == 1 and run.launch() == ("mfma", 1), run.launch()
        assert_bits(Y, expected(oracle, name, variant, 0.2, oracle_rows=edge), f"{name} {variant}")
    run.close()
    W.free()


def test_big_tiles_split_in_two(gpu, oracle, path):
    """M = 1024, N = 8192: 128 of the large tiles, K = 1100 split in 2 (9 + 9 blocks).  A wrong
    part at one k shows only in the rows whose wide entry sits there, so the whole output is
    compared with the float64 product; the oracle's loops run on sampled rows."""
    name = "big_split2"
    W, run = mfma_launcher(path, oracle, name)
    _, X, B, _ = case(oracle, name)
    M = X.shape[0]
    rows = np.unique(np.concatenate([[0, 127, 128, M - 1], np.random.default_rng(7).integers(0, M, 12)]))
    for variant in ("basic", "prelu_onthego"):
        Y = run(X, B, variant, 0.2)
        assert run.launch() == ("mfma", 2), run.launch()
        assert_bits(Y, expected(oracle, name, variant, 0.2, oracle_rows=rows), f"{name} {variant}")
    run.close()
    W.free()
