"""The backward pass on the device API: dX = G . W^T by tcsc_gpu_sgemm_t on a
transposed plan (every kernel family), and tcsc_gpu_prelu_backward (dZ and db).

W is K x N; its transposed plan has N rows and K columns, so "X" of that plan is
the upstream gradient G (M x N) and its output is dX (M x K)."""
import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    tcsc_amd.build()
    tcsc_amd.require_gpu()
    return torch


# path, M, K, N, density
CASES = [
    ("gather", 300, 777, 333, 0.05),
    ("split", 1024, 96, 4096, 0.05),  # few column groups: the gather splits K (here: N)
    ("small", 2, 700, 2048, 0.05),
    ("mfma", 256, 512, 1024, 0.5),
]
_data = {}


def case_data(oracle, name):
    """Inputs and oracle outputs of a case, computed once and shared (never modified)."""
    if name not in _data:
        _, M, K, N, density = next(c for c in CASES if c[0] == name)
        seed = 5000 + 10 * [c[0] for c in CASES].index(name)
        Wd = oracle.ternary((K, N), density, seed)
        WT = oracle.tcsc_from_dense(np.ascontiguousarray(Wd.T))
        zeros = np.zeros(K, np.float32)
        Gi, Gu = oracle.integers((M, N), seed + 1), oracle.uniform((M, N), seed + 2)
        d = dict(M=M, K=K, N=N, Wd=Wd, WT=WT, Gi=Gi, Gu=Gu, Xi=oracle.integers((M, K), seed + 3),
                 dXi=oracle.sgemm("basic", Gi, WT, zeros), f64=oracle.f64_rows(Gu, WT, zeros))
        _data[name] = d
    return _data[name]


def transposed_plan(monkeypatch, W, path, M, stream=0, **kw):
    """The transposed plan, on the path the case is about: the cost model's choice where
    it is that path, else created again under TCSC_PATH."""
    want = {"gather": "gather", "split": "gather", "small": "small", "mfma": "mfma"}[path]
    plan = tcsc_amd.Plan.transposed(W, stream=stream, **kw)
    plan.reserve(M)
    if plan.launch_info(M)[0] != want and want in ("gather", "mfma"):
        plan.destroy()
        monkeypatch.setenv("TCSC_PATH", want)
        plan = tcsc_amd.Plan.transposed(W, stream=stream, **kw)
        monkeypatch.delenv("TCSC_PATH")
        plan.reserve(M)
    got, slices = plan.launch_info(M)
    assert got == want, (got, slices)
    if path == "split":
        assert slices > 1, slices
    return plan


def run_sgemm_t(torch, plan, G, M, K, ldx=None):
    ldx = K if ldx is None else ldx
    dG = torch.from_numpy(np.ascontiguousarray(G)).to(DEV)
    dX = torch.full((M, ldx), -123.0, device=DEV)
    plan.sgemm_t(dG, dX, M, ldx, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dX.cpu().numpy()


@pytest.mark.parametrize("path", [c[0] for c in CASES])
def test_sgemm_t_on_every_path(torch_gpu, oracle, monkeypatch, path):
    d = case_data(oracle, path)
    M, K, N = d["M"], d["K"], d["N"]
    W = tcsc_amd.TcscMatrix.from_dense(d["Wd"])
    plan = transposed_plan(monkeypatch, W, path, M)
    info = plan.info()
    assert (info["rows"], info["cols"], info["col_begin"]) == (N, K, 0)
    assert info["nnz"] == d["WT"].nnz and info["device_bytes"] >= 4 * K
    # integer G: exact in any order
    dXi = run_sgemm_t(torch_gpu, plan, d["Gi"], M, K)
    np.testing.assert_array_equal(dXi.view(np.uint32), d["dXi"].view(np.uint32))
    # uniform G: the project's float bound against the exact sums
    dXu = run_sgemm_t(torch_gpu, plan, d["Gu"], M, K)
    ok, ratio = pyoracle.check_close(dXu, *d["f64"])
    print(f"{path}: worst err/bound {ratio:.3g}")
    assert ok, ratio
    # <G, X W> == <G W^T, X>, in integers, without the oracle
    Xi, Gi, Wi = d["Xi"].astype(np.int64), d["Gi"].astype(np.int64), d["Wd"].astype(np.int64)
    assert int((Gi * (Xi @ Wi)).sum()) == int((dXi.astype(np.int64) * Xi).sum())
    assert np.array_equal(dXi.astype(np.int64), dXi)  # the GPU values were integers
    plan.destroy()
    W.free()


def test_column_ranges_give_partial_dx(torch_gpu, oracle, monkeypatch):
    d = case_data(oracle, "gather")
    M, K, N = d["M"], d["K"], d["N"]
    W = tcsc_amd.TcscMatrix.from_dense(d["Wd"])
    zeros = np.zeros(K, np.float32)
    total = np.zeros((M, K), np.float32)
    for c0, c1 in ((0, 100), (100, N)):
        plan = tcsc_amd.Plan.transposed(W, c0, c1)
        info = plan.info()
        assert (info["rows"], info["cols"], info["col_begin"]) == (c1 - c0, K, 0)
        part = run_sgemm_t(torch_gpu, plan, d["Gi"][:, c0:c1], M, K)
        WTs = oracle.tcsc_from_dense(np.ascontiguousarray(d["Wd"][:, c0:c1].T))
        want = oracle.sgemm("basic", np.ascontiguousarray(d["Gi"][:, c0:c1]), WTs, zeros)
        np.testing.assert_array_equal(part.view(np.uint32), want.view(np.uint32))
        total += part
        plan.destroy()
    np.testing.assert_array_equal(total, d["dXi"])
    W.free()


def test_transposed_from_device_matches_the_host_constructor(torch_gpu, oracle):
    torch = torch_gpu
    d = case_data(oracle, "gather")
    M, K, N = d["M"], d["K"], d["N"]
    arrs = [torch.from_numpy(a).to(DEV) for a in oracle.tcsc_from_dense(d["Wd"]).arrays()]
    plan = tcsc_amd.Plan.transposed_from_device(K, N, *arrs)
    dXi = run_sgemm_t(torch, plan, d["Gi"], M, K)
    np.testing.assert_array_equal(dXi.view(np.uint32), d["dXi"].view(np.uint32))
    plan.destroy()


def test_ldx_padding_keeps_its_sentinel(torch_gpu, oracle):
    d = case_data(oracle, "gather")
    M, K = d["M"], d["K"]
    W = tcsc_amd.TcscMatrix.from_dense(d["Wd"])
    plan = tcsc_amd.Plan.transposed(W)
    out = run_sgemm_t(torch_gpu, plan, d["Gi"], M, K, ldx=K + 9)
    np.testing.assert_array_equal(out[:, :K].view(np.uint32), d["dXi"].view(np.uint32))
    assert (out[:, K:] == -123.0).all()
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)"):
        run_sgemm_t(torch_gpu, plan, d["Gi"], M, K, ldx=K - 1)
    plan.destroy()
    W.free()


def test_reference_order_is_bit_identical_on_floats(torch_gpu, oracle):
    d = case_data(oracle, "gather")
    M, K = d["M"], d["K"]
    W = tcsc_amd.TcscMatrix.from_dense(d["Wd"])
    tcsc_amd.set_order("reference")
    try:
        plan = tcsc_amd.Plan.transposed(W)
    finally:
        tcsc_amd.set_order("fast")
    assert plan.info()["order"] == 1
    got = run_sgemm_t(torch_gpu, plan, d["Gu"], M, K)
    want = oracle.sgemm("basic", d["Gu"], d["WT"], np.zeros(K, np.float32))
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    plan.destroy()
    W.free()


def test_sgemm_t_refuses_an_ordinary_plan(torch_gpu, oracle):
    torch = torch_gpu
    d = case_data(oracle, "gather")
    M, K, N = d["M"], d["K"], d["N"]
    W = tcsc_amd.TcscMatrix.from_dense(d["Wd"])
    plan = tcsc_amd.Plan(W)
    X = torch.zeros((M, K), device=DEV)
    Y = torch.zeros((M, N), device=DEV)
    with pytest.raises(tcsc_amd.TcscError, match="not a transposed plan"):
        plan.sgemm_t(X, Y, M, N)
    plan.destroy()
    W.free()


def test_graph_capture_of_the_backward_step(torch_gpu, oracle):
    """prelu_backward + sgemm_t captured on a side stream: after reserve(M) neither
    allocates nor synchronises, and every replay gives the eager launch's bits."""
    torch = torch_gpu
    d = case_data(oracle, "gather")
    M, K, N, a = d["M"], d["K"], d["N"], 0.2
    W = tcsc_amd.TcscMatrix.from_dense(d["Wd"])
    side = torch.cuda.Stream()
    plan = tcsc_amd.Plan.transposed(W, stream=side.cuda_stream)
    plan.reserve(M)
    need, reserved = plan.workspace(M)
    assert need <= reserved, (need, reserved)
    G = torch.from_numpy(d["Gu"]).to(DEV)
    Y = torch.from_numpy(oracle.uniform((M, N), 5900)).to(DEV)

    def step(dz, db, dx, s):
        tcsc_amd.prelu_backward(G, Y, a, dz, db, M, N, stream=s)
        plan.sgemm_t(dz, dx, M, K, s)

    eager = [torch.empty((M, N), device=DEV), torch.empty(N, device=DEV), torch.empty((M, K), device=DEV)]
    with torch.cuda.stream(side):
        step(*eager, side.cuda_stream)
    side.synchronize()
    want = [t.cpu().numpy().view(np.uint32) for t in eager]
    assert np.array_equal(eager[0].cpu().numpy(), np.where(Y.cpu().numpy() < 0, np.float32(a) * d["Gu"], d["Gu"]))
    outs = [torch.empty_like(t) for t in eager]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step(*outs, torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        for t in outs:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for t, w in zip(outs, want):
            np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), w)
    del g
    plan.destroy()
    W.free()


# ---- tcsc_gpu_prelu_backward ---------------------------------------------------

PITCHES = [(0, 0, 0), (0, 3, 8), (8, 0, 3), (3, 8, 0), (3, 3, 3), (8, 8, 8)]  # added to N for G, Y, dZ
SENT = -777.0


def padded(torch, a, ld):
    """`a` (M x N) in the first N columns of an M x ld device buffer of sentinels."""
    t = torch.full((a.shape[0], ld), SENT, device=DEV)
    t[:, :a.shape[1]] = torch.from_numpy(a)
    return t


def planted_y(oracle, M, N, seed):
    Y = oracle.uniform((M, N), seed)
    special = [-0.0, 0.0, np.nan, np.inf, -np.inf, -1e-30, -1e-40, 1e-40]
    flat = Y.reshape(-1)
    for i, v in enumerate(special):
        flat[(i * 7919) % flat.size] = v
    return Y


def db_bound_ok(db, dZ):
    d64 = dZ.astype(np.float64)
    bound = pyoracle.TOL_REL * np.abs(d64).sum(0) + pyoracle.TOL_ABS
    err = np.abs(db.astype(np.float64) - d64.sum(0))
    return bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("M,N", [(1, 1), (3, 5), (300, 333), (1000, 700)])
def test_prelu_backward(torch_gpu, oracle, M, N):
    torch = torch_gpu
    a = 0.2
    s = torch.cuda.current_stream().cuda_stream
    G = oracle.uniform((M, N), 6000 + M)
    Y = planted_y(oracle, M, N, 6001 + M)
    want = np.where(Y < 0, np.float32(a) * G, G)
    assert want.dtype == np.float32
    db_seen = []
    for pg, py, pz in PITCHES:
        ldg, ldy, lddz = N + pg, N + py, N + pz
        dG, dY = padded(torch, G, ldg), padded(torch, Y, ldy)
        dZ = torch.full((M, lddz), SENT, device=DEV)
        dB = torch.full((N + 2,), SENT, device=DEV)
        tcsc_amd.prelu_backward(dG, dY, a, dZ, dB, M, N, ldg, ldy, lddz, s)
        torch.cuda.synchronize()
        z = dZ.cpu().numpy()
        np.testing.assert_array_equal(z[:, :N].view(np.uint32), want.view(np.uint32), err_msg=str((pg, py, pz)))
        assert (z[:, N:] == SENT).all() and (dB[N:] == SENT).all()
        assert (dG[:, N:] == SENT).all() and (dY[:, N:] == SENT).all()
        np.testing.assert_array_equal(dG[:, :N].cpu().numpy().view(np.uint32), G.view(np.uint32))
        db = dB[:N].cpu().numpy()
        ok, ratio = db_bound_ok(db, want)
        assert ok, ratio
        db_seen.append(db.view(np.uint32).copy())
        # a second run: the same bits
        tcsc_amd.prelu_backward(dG, dY, a, dZ, dB, M, N, ldg, ldy, lddz, s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dB[:N].cpu().numpy().view(np.uint32), db_seen[-1])
        # dZ = None: only db, the same bits
        dB2 = torch.full((N,), SENT, device=DEV)
        tcsc_amd.prelu_backward(dG, dY, a, None, dB2, M, N, ldg, ldy, stream=s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dB2.cpu().numpy().view(np.uint32), db_seen[-1])
        # in place (dZ is G), db = None
        tcsc_amd.prelu_backward(dG, dY, a, dG, None, M, N, ldg, ldy, ldg, s)
        torch.cuda.synchronize()
        g2 = dG.cpu().numpy()
        np.testing.assert_array_equal(g2[:, :N].view(np.uint32), want.view(np.uint32))
        assert (g2[:, N:] == SENT).all()
    # the summation order does not depend on pitches or on the vector / scalar path
    for other in db_seen[1:]:
        np.testing.assert_array_equal(other, db_seen[0])


@pytest.mark.parametrize("M,N", [(3, 5), (1000, 700)])
def test_prelu_backward_identity_activation(torch_gpu, oracle, M, N):
    torch = torch_gpu
    G = oracle.uniform((M, N), 6100 + M)
    dG = torch.from_numpy(G).to(DEV)
    dZ = torch.full((M, N), SENT, device=DEV)
    dB = torch.full((N,), SENT, device=DEV)
    tcsc_amd.prelu_backward(dG, None, 0.2, dZ, dB, M, N, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dZ.cpu().numpy().view(np.uint32), G.view(np.uint32))
    ok, ratio = db_bound_ok(dB.cpu().numpy(), G)
    assert ok, ratio


@pytest.mark.parametrize("M,N", [(1, 1), (3, 5), (300, 333), (1000, 700)])
def test_prelu_backward_db_exact_on_even_integers(torch_gpu, oracle, M, N):
    torch = torch_gpu
    a = 0.5
    G = 2.0 * oracle.integers((M, N), 6200 + M)
    Y = planted_y(oracle, M, N, 6201 + M)
    want = np.where(Y < 0, np.float32(a) * G, G).astype(np.int64)
    dB = torch.full((N,), SENT, device=DEV)
    tcsc_amd.prelu_backward(torch.from_numpy(G).to(DEV), torch.from_numpy(Y).to(DEV), a, None, dB, M, N,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    db = dB.cpu().numpy()
    np.testing.assert_array_equal(db.astype(np.int64), want.sum(0))
    assert np.array_equal(db.astype(np.int64), db)


def test_prelu_backward_degenerate_shapes(torch_gpu):
    torch = torch_gpu
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.full((8,), SENT, device=DEV)
    tcsc_amd.prelu_backward(buf, buf, 0.2, buf, buf, 3, 0, stream=s)  # N == 0: nothing
    torch.cuda.synchronize()
    assert (buf == SENT).all()
    tcsc_amd.prelu_backward(buf, buf, 0.2, buf, buf, 0, 5, stream=s)  # M == 0: db = the empty sum
    torch.cuda.synchronize()
    assert (buf[:5] == 0).all() and (buf[5:] == SENT).all()
