"""k_stream_w, the 22-column geometry (tcsc_wide.hip), against k_stream.

Every case runs the same plan and the same float inputs twice, TCSC_GEO=16
and TCSC_GEO=22 (read per launch), and asks for the same bits: both kernels
add each column's nonzeros in ascending k and the bias after the sum.  The
22-column result is also held to the suite's bound against the fp64 oracle.
The plan is reserved under TCSC_GEO=22, which builds the wide streams from
the plan's own 16-column streams.  TCSC_PATH=gather pins the gather and
TCSC_SLICES=1 keeps the 16-column launch unsplit like the 22-column one.
"""
import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu
A = 0.2


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    tcsc_amd.build()
    tcsc_amd.require_gpu()
    return torch


@pytest.fixture(autouse=True)
def gather_only(monkeypatch):
    monkeypatch.setenv("TCSC_PATH", "gather")
    # the 16-column launch unsplit too: a K split sums in another order
    monkeypatch.setenv("TCSC_SLICES", "1")
    for k in ("TCSC_ORDER", "TCSC_GEO"):
        monkeypatch.delenv(k, raising=False)


def wide_plan(monkeypatch, W, max_M, col_begin=0, col_end=None):
    monkeypatch.setenv("TCSC_GEO", "22")
    plan = tcsc_amd.Plan(W, col_begin, col_end)
    plan.reserve(max_M)
    return plan


def both(monkeypatch, torch, plan, launch, M, N, ldy):
    """launch(Y) under each geometry into NaN-filled M x ldy buffers."""
    out = {}
    for geo in (16, 22):
        monkeypatch.setenv("TCSC_GEO", str(geo))
        assert plan.launch_geometry(M) == geo
        Y = torch.full((M, ldy), float("nan"), device="cuda")
        launch(Y)
        torch.cuda.synchronize()
        out[geo] = Y.cpu().numpy()
    return out[16], out[22]


def same_bits(y16, y22, N):
    assert np.array_equal(y16[:, :N].view(np.uint32), y22[:, :N].view(np.uint32))
    assert np.isnan(y22[:, N:]).all(), "columns past N (ldy > N) were written"


def dense_w(oracle, K, N, density, seed, empty=()):
    Wd = oracle.ternary((K, N), density, seed) if density > 0 else np.zeros((K, N), np.float32)
    for lo, hi in empty:
        Wd[:, lo:hi] = 0.0
    return Wd


# id, M, K, N, density, empty column ranges
SHAPES = [
    ("one_block_one_chunk", 64, 48, 352, 0.05, ()),
    ("ragged_rows_k_8col_tail", 260, 100, 360, 0.05, ()),
    ("two_blocks", 256, 96, 704, 0.05, ()),
    ("m300_k1000_n1000", 300, 1000, 1000, 0.05, ()),
    ("dense_streams_reload", 256, 200, 352, 0.50, ()),
    ("all_zero_w", 70, 100, 400, 0.0, ()),
    # a whole wave's 22 columns, a run across a block boundary, the last column
    ("empty_columns", 130, 150, 800, 0.10, ((22, 44), (340, 370), (799, 800))),
]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c[0])
def test_wide_bits_equal_narrow(torch_gpu, oracle, monkeypatch, case):
    torch = torch_gpu
    _, M, K, N, density, empty = case
    Wd = dense_w(oracle, K, N, density, 31, empty)
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    X, B = oracle.uniform((M, K), 32), oracle.uniform((N,), 33)
    dX, dB = torch.from_numpy(X).cuda(), torch.from_numpy(B).cuda()
    plan = wide_plan(monkeypatch, W, M)
    y16, y22 = both(monkeypatch, torch, plan, lambda Y: plan.sgemm(dX, dB, Y, M, N, "prelu_basic", A), M, N, N)
    same_bits(y16, y22, N)
    Y64, S64 = oracle.f64_rows(X, oracle.tcsc_from_dense(Wd), B)
    ok, ratio = pyoracle.check_close(y22, Y64, S64, A)
    assert ok, f"worst err/bound {ratio:.3g}"
    plan.destroy()
    W.free()


@pytest.fixture(scope="module")
def mid(oracle):
    """One ragged shape shared by the variant / pitch / entry-point cases."""
    M, K, N = 200, 120, 500
    Wd = oracle.ternary((K, N), 0.08, 41)
    X, B = oracle.uniform((M, K), 42), oracle.uniform((N,), 43)
    Wref = oracle.tcsc_from_dense(Wd)
    Y64, S64 = oracle.f64_rows(X, Wref, B)
    return dict(M=M, K=K, N=N, Wd=Wd, X=X, B=B, Wref=Wref, Y64=Y64, S64=S64)


# the fast order adds the bias after the sum for every variant; `basic` is the
# variant whose reference adds it first (that order never takes this kernel)
@pytest.mark.parametrize("variant", ["basic", "optimized", "prelu_basic", "prelu_onthego", "sparse_gemm"])
def test_wide_every_variant(torch_gpu, oracle, monkeypatch, mid, variant):
    torch = torch_gpu
    M, N = mid["M"], mid["N"]
    W = tcsc_amd.TcscMatrix.from_dense(mid["Wd"])
    dX, dB = torch.from_numpy(mid["X"]).cuda(), torch.from_numpy(mid["B"]).cuda()
    plan = wide_plan(monkeypatch, W, M)
    y16, y22 = both(monkeypatch, torch, plan, lambda Y: plan.sgemm(dX, dB, Y, M, N, variant, A), M, N, N)
    same_bits(y16, y22, N)
    ok, ratio = pyoracle.check_close(y22, mid["Y64"], mid["S64"], A if variant in tcsc_amd.PRELU_VARIANTS else None)
    assert ok, f"worst err/bound {ratio:.3g}"
    plan.destroy()
    W.free()


@pytest.mark.parametrize("pad", [8, 3], ids=["ldy_quads", "ldy_odd"])
def test_wide_ldy_larger_than_n(torch_gpu, oracle, monkeypatch, mid, pad):
    """ldy > N: whole-quad stores (ldy % 4 == 0) and the scalar stores."""
    torch = torch_gpu
    M, N = mid["M"], mid["N"]
    W = tcsc_amd.TcscMatrix.from_dense(mid["Wd"])
    dX, dB = torch.from_numpy(mid["X"]).cuda(), torch.from_numpy(mid["B"]).cuda()
    plan = wide_plan(monkeypatch, W, M)
    y16, y22 = both(monkeypatch, torch, plan, lambda Y: plan.sgemm(dX, dB, Y, M, N + pad, "prelu_basic", A), M, N,
                    N + pad)
    same_bits(y16, y22, N)
    ok, ratio = pyoracle.check_close(y22[:, :N], mid["Y64"], mid["S64"], A)
    assert ok, f"worst err/bound {ratio:.3g}"
    plan.destroy()
    W.free()


def test_wide_column_block_plan(torch_gpu, oracle, monkeypatch, mid):
    """A plan over columns [90, 471) of W: col_begin > 0, 381 columns."""
    torch = torch_gpu
    M, c0, c1 = mid["M"], 90, 471
    n = c1 - c0
    W = tcsc_amd.TcscMatrix.from_dense(mid["Wd"])
    dX, dB = torch.from_numpy(mid["X"]).cuda(), torch.from_numpy(mid["B"][c0:c1].copy()).cuda()
    plan = wide_plan(monkeypatch, W, M, c0, c1)
    y16, y22 = both(monkeypatch, torch, plan, lambda Y: plan.sgemm(dX, dB, Y, M, n, "prelu_basic", A), M, n, n)
    same_bits(y16, y22, n)
    ok, ratio = pyoracle.check_close(y22, mid["Y64"][:, c0:c1], mid["S64"][:, c0:c1], A)
    assert ok, f"worst err/bound {ratio:.3g}"
    plan.destroy()
    W.free()


def test_wide_prepared_path(torch_gpu, oracle, monkeypatch, mid):
    torch = torch_gpu
    M, N = mid["M"], mid["N"]
    W = tcsc_amd.TcscMatrix.from_dense(mid["Wd"])
    dX, dB = torch.from_numpy(mid["X"]).cuda(), torch.from_numpy(mid["B"]).cuda()
    plan = wide_plan(monkeypatch, W, M)
    plan.prepare_x(dX, M)
    y16, y22 = both(monkeypatch, torch, plan, lambda Y: plan.sgemm_prepared(dB, Y, M, N, "prelu_basic", A), M, N, N)
    same_bits(y16, y22, N)
    ok, ratio = pyoracle.check_close(y22, mid["Y64"], mid["S64"], A)
    assert ok, f"worst err/bound {ratio:.3g}"
    plan.destroy()
    W.free()


def test_wide_bf16_and_i8_entry_points(torch_gpu, oracle, monkeypatch, mid):
    torch = torch_gpu
    M, K, N = mid["M"], mid["K"], mid["N"]
    W = tcsc_amd.TcscMatrix.from_dense(mid["Wd"])
    dB = torch.from_numpy(mid["B"]).cuda()
    plan = wide_plan(monkeypatch, W, M)
    Xb = torch.from_numpy(mid["X"]).cuda().to(torch.bfloat16)
    y16, y22 = both(monkeypatch, torch, plan, lambda Y: plan.sgemm_bf16(Xb, dB, Y, M, N, "prelu_basic", A), M, N, N)
    same_bits(y16, y22, N)
    Y64, S64 = oracle.f64_rows(Xb.float().cpu().numpy(), mid["Wref"], mid["B"])
    ok, ratio = pyoracle.check_close(y22, Y64, S64, A)
    assert ok, f"bf16: worst err/bound {ratio:.3g}"
    Xq = torch.randint(-127, 128, (M, K), dtype=torch.int8, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    scale = torch.rand(M, device="cuda", generator=torch.Generator("cuda").manual_seed(6)) * 0.01 + 0.001
    y16, y22 = both(monkeypatch, torch, plan, lambda Y: plan.sgemm_i8(Xq, scale, dB, Y, M, N, "prelu_basic", A), M, N,
                    N)
    same_bits(y16, y22, N)
    Y64, S64 = oracle.f64_rows((scale[:, None] * Xq.float()).cpu().numpy(), mid["Wref"], mid["B"])
    ok, ratio = pyoracle.check_close(y22, Y64, S64, A)
    assert ok, f"i8: worst err/bound {ratio:.3g}"
    plan.destroy()
    W.free()


def test_wide_refused_where_it_cannot_run(torch_gpu, oracle, monkeypatch, mid):
    """TCSC_GEO=22 with a forced K split, or on a reference-order plan: the usual error."""
    torch = torch_gpu
    M, N = mid["M"], mid["N"]
    W = tcsc_amd.TcscMatrix.from_dense(mid["Wd"])
    dX, dB = torch.from_numpy(mid["X"]).cuda(), torch.from_numpy(mid["B"]).cuda()
    Y = torch.empty((M, N), device="cuda")
    plan = wide_plan(monkeypatch, W, M)
    monkeypatch.setenv("TCSC_SLICES", "2")
    with pytest.raises(tcsc_amd.TcscError, match="TCSC_GEO=22"):
        plan.sgemm(dX, dB, Y, M, N, "prelu_basic", A)
    monkeypatch.setenv("TCSC_SLICES", "1")
    plan.destroy()
    tcsc_amd.set_order("reference")
    try:
        ref = tcsc_amd.Plan(W)
        ref.reserve(M)
        with pytest.raises(tcsc_amd.TcscError, match="TCSC_GEO=22"):
            ref.sgemm(dX, dB, Y, M, N, "prelu_basic", A)
        ref.destroy()
    finally:
        tcsc_amd.set_order("fast")
    torch.cuda.synchronize()
    W.free()


def test_wide_reserve_contract(torch_gpu, oracle, monkeypatch, mid):
    """reserve(max_M) builds the wide streams and counts them; afterwards launches
    of any M <= max_M leave device_bytes alone and one of them can be captured."""
    torch = torch_gpu
    K, N, max_M = mid["K"], mid["N"], 600
    W = tcsc_amd.TcscMatrix.from_dense(mid["Wd"])
    X = oracle.uniform((max_M, K), 44)
    dX, dB = torch.from_numpy(X).cuda(), torch.from_numpy(mid["B"]).cuda()
    side = torch.cuda.Stream()
    monkeypatch.setenv("TCSC_GEO", "16")
    narrow = tcsc_amd.Plan(W)
    narrow.reserve(max_M)
    monkeypatch.setenv("TCSC_GEO", "22")
    plan = tcsc_amd.Plan(W)
    plan.reserve(max_M)
    bytes0 = plan.info()["device_bytes"]
    extra = bytes0 - narrow.info()["device_bytes"]
    nnz = W.nnz
    # about one more copy of the entry streams: 8 B per nonzero + headers and offsets per (group, chunk)
    assert 8 * nnz <= extra <= 8 * nnz + 16384, extra
    Y64, S64 = oracle.f64_rows(X, mid["Wref"], mid["B"])
    for M in (600, 257, 256, 64, 5):
        assert plan.launch_geometry(M) == 22
        Y = torch.empty((M, N), device="cuda")
        plan.sgemm(dX, dB, Y, M, N, "prelu_basic", A)
        torch.cuda.synchronize()
        assert plan.info()["device_bytes"] == bytes0, M
        ok, ratio = pyoracle.check_close(Y.cpu().numpy(), Y64[:M], S64[:M], A)
        assert ok, f"M={M}: worst err/bound {ratio:.3g}"
    M = 300
    Ye, Yg = torch.empty((M, N), device="cuda"), torch.zeros((M, N), device="cuda")
    plan.sgemm(dX, dB, Ye, M, N, "prelu_basic", A)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm(dX, dB, Yg, M, N, "prelu_basic", A, torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(Ye, Yg)
    assert plan.info()["device_bytes"] == bytes0
    plan.destroy()
    narrow.destroy()
    W.free()
