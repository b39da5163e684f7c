"""The slot map of the 22-column geometry (k_wide_balance, tcsc_wide.hip).

tcsc_gpu_plan_reserve deals every full 352-column block's columns to the
block's 16 waves so that the busiest wave of a chunk has fewer entries; the
kernel's chunk loop is the same, the streams and the epilogue's parking follow
the map.  Every case runs one launch three ways -- TCSC_GEO=16, TCSC_GEO=22 on
a plan reserved under TCSC_WIDE_BALANCE=1 (the default) and TCSC_GEO=22 on a
plan reserved under TCSC_WIDE_BALANCE=0 (the identity map) -- and asks for the
same bits, holds the result to the suite's bound against the fp64 oracle,
checks the map (a bijection per block, 22 slots per wave, the identity on a
partial block) and recomputes tcsc_gpu_plan_wide_stats's four numbers from W
and the returned map in numpy.
"""
import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu
A = 0.2
WAVES, CW, WG = 16, 22, 352
CAP = 30  # TCSCW_GEN_CAP, the wide loop's scalar entry buffer (tests/test_wide_geometry.py WIDE)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    tcsc_amd.build()
    tcsc_amd.require_gpu()
    return torch


@pytest.fixture(autouse=True)
def gather_only(monkeypatch):
    monkeypatch.setenv("TCSC_PATH", "gather")
    monkeypatch.setenv("TCSC_SLICES", "1")  # the 16-column launch unsplit too: a K split sums in another order
    for k in ("TCSC_ORDER", "TCSC_GEO", "TCSC_WIDE_BALANCE"):
        monkeypatch.delenv(k, raising=False)


def wide_plan(monkeypatch, W, max_M, balance, col_begin=0, col_end=None):
    monkeypatch.setenv("TCSC_GEO", "22")
    monkeypatch.setenv("TCSC_WIDE_BALANCE", "1" if balance else "0")
    plan = tcsc_amd.Plan(W, col_begin, col_end)
    plan.reserve(max_M)
    monkeypatch.delenv("TCSC_WIDE_BALANCE")
    return plan


def run(monkeypatch, torch, plan, geo, launch, M, ldy):
    monkeypatch.setenv("TCSC_GEO", str(geo))
    assert plan.launch_geometry(M) == geo
    Y = torch.full((M, ldy), float("nan"), device="cuda")
    launch(plan, Y)
    torch.cuda.synchronize()
    return Y.cpu().numpy()


def recompute(Wd, chunk_k, m):
    """(max_identity, max_map, long_identity, long_map) of map m over the columns of Wd."""
    K, n = Wd.shape
    nch, nblk = -(-K // chunk_k), -(-n // WG)
    nz = np.zeros((nch * chunk_k, nblk * WG), np.int64)
    nz[:K, :n] = Wd != 0
    cnt = nz.reshape(nch, chunk_k, nblk, WG).sum(axis=1)  # [chunk, block, column in block]
    out = []
    for mp in (np.arange(WG).reshape(1, WAVES, CW).repeat(nblk, 0), m.astype(np.int64)):
        L = np.stack([cnt[:, b, :][:, mp[b]].sum(axis=2) for b in range(nblk)])  # [block, chunk, wave]
        out.append((int(L.max(axis=2).sum()), int((L > CAP).sum())))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def check_map(m, ncols):
    nblk = -(-ncols // WG)
    assert m.shape == (nblk, WAVES, CW) and m.dtype == np.uint16
    ident = np.arange(WG).reshape(WAVES, CW)
    for b in range(nblk):
        assert np.array_equal(np.sort(m[b].ravel()), np.arange(WG)), f"block {b} is no bijection"
        if (b + 1) * WG > ncols:
            assert np.array_equal(m[b], ident), "a partial block keeps the identity"
    return not all(np.array_equal(m[b], ident) for b in range(nblk))


def case_w(oracle, name):
    if name == "one_block_one_chunk":
        return 64, oracle.ternary((48, 352), 0.05, 51)
    if name == "two_blocks_40_chunks":
        return 260, oracle.ternary((1920, 704), 0.02, 52)
    if name == "identity_tail_8":
        return 130, oracle.ternary((150, 360), 0.05, 53)
    if name == "heavy_wave":
        Wd = oracle.ternary((200, 352), 0.01, 54)
        Wd[:, :22] = oracle.ternary((200, 22), 0.50, 55)
        return 256, Wd
    if name == "empty_columns":
        Wd = oracle.ternary((150, 800), 0.10, 56)
        for lo, hi in ((22, 44), (340, 370), (799, 800)):
            Wd[:, lo:hi] = 0.0
        return 130, Wd
    raise KeyError(name)


CASES = ["one_block_one_chunk", "two_blocks_40_chunks", "identity_tail_8", "heavy_wave", "empty_columns"]


def compare(monkeypatch, torch, oracle, Wd, M, c0, c1, pad, seed):
    """The three launches of the plan over columns [c0, c1) of Wd; returns the balanced plan's statistics."""
    K, n = Wd.shape[0], c1 - c0
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    X, B = oracle.uniform((M, K), seed), oracle.uniform((n,), seed + 1)
    dX, dB = torch.from_numpy(X).cuda(), torch.from_numpy(B).cuda()
    bal = wide_plan(monkeypatch, W, M, True, c0, c1)
    idn = wide_plan(monkeypatch, W, M, False, c0, c1)

    def launch(plan, Y):
        plan.sgemm(dX, dB, Y, M, n + pad, "prelu_basic", A)

    y16 = run(monkeypatch, torch, bal, 16, launch, M, n + pad)
    y22 = run(monkeypatch, torch, bal, 22, launch, M, n + pad)
    y22i = run(monkeypatch, torch, idn, 22, launch, M, n + pad)
    for y in (y22, y22i):
        assert np.array_equal(y16[:, :n].view(np.uint32), y[:, :n].view(np.uint32))
        assert np.isnan(y[:, n:]).all(), "columns past N (ldy > N) were written"
    Wcols = np.ascontiguousarray(Wd[:, c0:c1])
    Y64, S64 = oracle.f64_rows(X, oracle.tcsc_from_dense(Wcols), B)
    ok, ratio = pyoracle.check_close(y22[:, :n], Y64, S64, A)
    assert ok, f"worst err/bound {ratio:.3g}"
    chunk_k = bal.info()["chunk_k"]
    sb, si = bal.wide_stats(), idn.wide_stats()
    sb["permuted"] = check_map(sb["map"], n)
    assert not check_map(si["map"], n), "TCSC_WIDE_BALANCE=0 keeps the identity"
    for s in (sb, si):
        got = (s["max_identity"], s["max_balanced"], s["long_identity"], s["long_balanced"])
        want = recompute(Wcols, chunk_k, s["map"])
        print(f"wide_stats n={n} K={K}: library {got} numpy {want}")
        assert got == want
    assert si["max_balanced"] == si["max_identity"] == sb["max_identity"]
    assert sb["max_balanced"] <= sb["max_identity"]
    if sb["permuted"]:  # a deal is kept only where it is strictly better
        assert sb["max_balanced"] < sb["max_identity"]
    bal.destroy()
    idn.destroy()
    W.free()
    return sb


@pytest.mark.parametrize("name", CASES)
def test_balanced_bits_map_and_stats(torch_gpu, oracle, monkeypatch, name):
    M, Wd = case_w(oracle, name)
    s = compare(monkeypatch, torch_gpu, oracle, Wd, M, 0, Wd.shape[1], 0, 60)
    if name in ("two_blocks_40_chunks", "heavy_wave"):
        assert s["permuted"], "the map is the identity: the case proves nothing"
    if name == "two_blocks_40_chunks":
        # the greedy deal alone gives 0.83-0.85 on iid counts of this shape (six seeds, simulated); the identity 1.0
        print(f"balanced / identity = {s['max_balanced'] / s['max_identity']:.4f}")
        assert s["max_balanced"] <= 0.90 * s["max_identity"]


@pytest.fixture(scope="module")
def mid(oracle):
    return oracle.ternary((120, 500), 0.08, 41)


def test_balanced_column_block_plan(torch_gpu, oracle, monkeypatch, mid):
    """A plan over columns [90, 471) of W: one full block of the plan's own columns and a tail of 29."""
    compare(monkeypatch, torch_gpu, oracle, mid, 200, 90, 471, 0, 62)


def test_balanced_ldy_odd(torch_gpu, oracle, monkeypatch):
    """ldy = N + 3: the epilogue's scalar stores."""
    M, Wd = case_w(oracle, "identity_tail_8")
    compare(monkeypatch, torch_gpu, oracle, Wd, M, 0, Wd.shape[1], 3, 64)


def test_balanced_reserve_contract(torch_gpu, oracle, monkeypatch, mid):
    """The map is built by reserve and counted in device_bytes, inside the bound the wide copy had before it;
    launches of five M leave device_bytes alone and one of them can be captured in a graph."""
    torch = torch_gpu
    (K, N), max_M = mid.shape, 600
    W = tcsc_amd.TcscMatrix.from_dense(mid)
    X, B = oracle.uniform((max_M, K), 44), oracle.uniform((N,), 43)
    dX, dB = torch.from_numpy(X).cuda(), torch.from_numpy(B).cuda()
    side = torch.cuda.Stream()
    monkeypatch.setenv("TCSC_GEO", "16")
    narrow = tcsc_amd.Plan(W)
    narrow.reserve(max_M)
    with pytest.raises(tcsc_amd.TcscError, match="no wide streams"):
        narrow.wide_stats()
    plan = wide_plan(monkeypatch, W, max_M, True)
    bytes0 = plan.info()["device_bytes"]
    extra = bytes0 - narrow.info()["device_bytes"]
    assert 8 * W.nnz <= extra <= 8 * W.nnz + 16384, extra
    Y64, S64 = oracle.f64_rows(X, oracle.tcsc_from_dense(mid), B)
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
