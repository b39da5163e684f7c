"""The state a plan carries from one launch to the next: its workspace.

include/tcsc_gpu.h promises that tcsc_gpu_plan_reserve(max_M) keeps every
launch of M <= max_M rows allocation-free (and so capturable in a hipGraph).
Both cost models split K more at smaller M (fewer row tiles to fill the CUs),
so slices x M x N can peak well below max_M; a reserve sized at max_M alone
leaves holes, and tcsc_gpu_sgemm then reallocates behind the caller's back:
it synchronises the device, fails under capture, and leaves an earlier graph
holding a freed pointer.

The first two tests are host arithmetic on a live plan through
Plan.workspace (tcsc_gpu_plan_workspace): exhaustive over M, no launches.
The others launch a sequence of different M on one plan and compare each
result with a fresh plan reserved at exactly that M, with the oracle, and
with a graph replay.
"""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

PATHS = (None, "gather", "mfma", "small")


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    tcsc_amd.build()
    tcsc_amd.require_gpu()
    return torch


@functools.lru_cache(maxsize=2)
def strided_arrays(K, N, density):
    """TCSC arrays of a regular K x N ternary pattern, built without a dense
    matrix: floor(density * K * N) nonzeros in all, spread evenly over the
    columns (column j holds floor((j + 1) density K) - floor(j density K) of
    them), at rows offset + i * step with offset = j % step, signs alternating."""
    per = density * K
    ends = np.floor(np.arange(N + 1, dtype=np.float64) * per).astype(np.int64)
    count = np.diff(ends)
    cmax = int(count.max())
    step = K // cmax
    i = np.arange(cmax, dtype=np.int64)[None, :]
    rows = (np.arange(N, dtype=np.int64) % step)[:, None] + i * step  # ascending along each column's list
    assert rows.max() < K
    held = i < count[:, None]
    pos, neg = held & (i % 2 == 0), held & (i % 2 == 1)
    csp = np.concatenate([[0], np.cumsum(pos.sum(1))]).astype(np.int32)
    csn = np.concatenate([[0], np.cumsum(neg.sum(1))]).astype(np.int32)
    return csp, csn, rows[pos].astype(np.int32), rows[neg].astype(np.int32)


def strided_w(K, N, density):
    return tcsc_amd.TcscMatrix.from_arrays(K, N, *strided_arrays(K, N, density))


def sweep(plan, max_M):
    """need[path][M] for M = 0 .. max_M through the query (need[.][0] = 0)."""
    need = {p: np.zeros(max_M + 1, np.int64) for p in PATHS}
    for M in range(1, max_M + 1):
        for p in PATHS:
            need[p][M] = plan.workspace(M, p)[0]
    return need


# (density, K, N, max_M, environment at plan creation and reserve)
GATHER_HOLES = [(0.02, 512, 4096, 512, {}), (0.02, 768, 4096, 1024, {}), (0.05, 512, 1024, 4096, {})]
MFMA_HOLES = [(0.06, 8192, 12288, 128, {}), (0.06, 8192, 12288, 256, {})]
CONTROLS = [(0.05, 1024, 96, 1024, {}), (0.5, 1024, 512, 256, {})]
FORCED = [(0.02, 512, 4096, 512, {"TCSC_SLICES": s}) for s in ("2", "3", "7")] + \
         [(0.5, 1024, 512, 256, {"TCSC_PATH": p}) for p in ("mfma", "gather")]
XT_DOMINATES = [(0.02, 2048, 2048, 4096, {})]  # X^T is most of the workspace: "16 slices always" over-reserves
SHAPES = GATHER_HOLES + MFMA_HOLES + CONTROLS + FORCED + XT_DOMINATES


def shape_id(s):
    d, K, N, max_M, env = s
    return f"d{d}-K{K}-N{N}-M{max_M}" + "".join(f"-{k[5:].lower()}{v}" for k, v in env.items())


def reserved_plan(monkeypatch, shape):
    d, K, N, max_M, env = shape
    for k in ("TCSC_SLICES", "TCSC_PATH", "TCSC_SMALL_M", "TCSC_MFMA_WGS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    W = strided_w(K, N, d)
    plan = tcsc_amd.Plan(W)
    assert plan.workspace(1)[1] == 0  # no prior workspace
    plan.reserve(max_M)
    return W, plan


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_reserve_covers_every_m(torch_gpu, monkeypatch, shape):
    """After reserve(max_M) every M <= max_M fits: the path the launch takes
    and every path the plan has (a forced path or slice count may differ
    between the reserve and the launch only through the environment, which
    the test keeps fixed).

    Measured with the reserve that sized the gather at max_M only and the MFMA
    path at multiples of 128 rows only (bytes needed at the worst M against
    bytes reserved):
      d0.02 K512  N4096  max_M 512:   M = 5 .. 339 too large,    17,940,480 at M = 339  against  1,277,952
      d0.02 K768  N4096  max_M 1024:  M = 11 .. 565,             39,682,048 at M = 565  against  3,538,944
      d0.05 K512  N1024  max_M 4096:  M = 213 .. 2970,           44,163,072 at M = 2970 against 10,223,616
      d0.02 K2048 N2048  max_M 4096:  M = 421 .. 3482,           88,014,848 at M = 3482 against 35,389,440
      d0.06 K8192 N12288 max_M 128:   M = 48 .. 64 (MFMA narrow tiles, 16 slices), 53,477,632 against 39,960,576
    and no hole on the other shapes (max_M 256 of the last one: the gather's
    71,417,856 at M = 256 covered the MFMA path's 53,477,632 at M = 64)."""
    d, K, N, max_M, env = shape
    W, plan = reserved_plan(monkeypatch, shape)
    need = sweep(plan, max_M)
    reserved = plan.workspace(max_M)[1]
    print(f"{shape_id(shape)}: reserved {reserved}")
    for p in PATHS:
        over = np.flatnonzero(need[p] > reserved)
        worst = int(np.argmax(need[p]))
        print(f"  path {p}: max need {int(need[p].max())} at M={worst}; "
              f"{over.size} M exceed the reserve" + (f" (M={over[0]}..{over[-1]})" if over.size else ""))
    for p in PATHS:
        over = np.flatnonzero(need[p] > reserved)
        assert over.size == 0, (f"path {p}: {over.size} values of M in {over[0]}..{over[-1]} need more than the "
                                f"{reserved} bytes reserve({max_M}) holds; worst M={int(np.argmax(need[p]))} "
                                f"needs {int(need[p].max())}")
    plan.destroy()
    W.free()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_reserve_does_not_over_reserve(torch_gpu, monkeypatch, shape):
    """reserve(max_M) on a plan without a workspace holds no more than the
    largest per-path need over M <= max_M (brute force through the query)."""
    d, K, N, max_M, env = shape
    W, plan = reserved_plan(monkeypatch, shape)
    need = sweep(plan, max_M)
    reserved = plan.workspace(max_M)[1]
    top = max(int(need[p].max()) for p in PATHS)
    print(f"{shape_id(shape)}: reserved {reserved}, largest need {top}")
    assert 0 < reserved <= top
    plan.destroy()
    W.free()


def test_query_rejects_bad_arguments_and_reports_absent_paths(torch_gpu, monkeypatch):
    W, plan = reserved_plan(monkeypatch, (0.02, 512, 4096, 512, {}))
    assert plan.info()["mfma_min_M"] == 0
    assert plan.workspace(64, "mfma")[0] == 0  # gather-only plan
    assert plan.workspace(5, "small")[0] == 0 and plan.workspace(4, "small")[0] == 4 * 512 * 4
    assert plan.workspace(0)[0] == 0
    for M in (1, 4, 5, 300):
        path = plan.launch_info(M)[0]
        assert plan.workspace(M) == plan.workspace(M, path)
    L = tcsc_amd.lib()
    assert L.tcsc_gpu_plan_workspace(plan.handle, -1, -1, None, None) == 1
    assert L.tcsc_gpu_plan_workspace(plan.handle, 8, 1, None, None) == 1  # the retired path
    assert L.tcsc_gpu_plan_workspace(None, 8, -1, None, None) == 1
    assert L.tcsc_gpu_plan_workspace(plan.handle, 8, -1, None, None) == 0
    plan.destroy()
    W.free()


# ---- what the cost models decide ---------------------------------------------

def load_gen_routing():
    """tests/golden/gen_routing.py: the plans and the record the table was made with."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_routing.py")
    spec = importlib.util.spec_from_file_location("gen_routing", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN_ROUTING = load_gen_routing()


@pytest.mark.parametrize("shape", GEN_ROUTING.SHAPES, ids=lambda s: f"K{s[0]}-N{s[1]}")
def test_routing_and_workspace_equal_the_recorded_table(torch_gpu, monkeypatch, shape):
    """tests/golden/routing_table.json holds, for fast-order plans of four shapes at six densities, with and
    without the int8 image, and 17 values of M: the path and K split of the fp32, bf16 and int8 calls, the
    workspace of the auto path and of each path, the gather geometry, and what reserve(4096) holds -- recorded
    once from the three per-type cost models and workspace layouts.  Every entry must be what it was."""
    for k in GEN_ROUTING.KNOBS:
        monkeypatch.delenv(k, raising=False)
    with open(GEN_ROUTING.TABLE) as f:
        table = json.load(f)
    got = GEN_ROUTING.record(tcsc_amd, *shape)
    assert len(got) == 2 * len(GEN_ROUTING.DENSITIES) and set(got) <= set(table)
    names = ("M", "path", "slices", "bf16 path", "bf16 slices", "i8 path", "i8 slices", "workspace", "gather ws",
             "mfma ws", "small ws", "geometry")
    for key, g in got.items():
        want = table[key]
        assert g["reserved"] == want["reserved"], f"{key}: reserve({GEN_ROUTING.RESERVE_M})"
        assert len(g["rows"]) == len(want["rows"]) == len(GEN_ROUTING.MS)
        for grow, wrow in zip(g["rows"], want["rows"]):
            assert grow == wrow, f"{key} M={wrow[0]}: " + ", ".join(
                f"{n} {a} (recorded {b})" for n, a, b in zip(names, grow, wrow) if a != b)


@pytest.mark.parametrize("name", list(GEN_ROUTING.KNOB_PLANS))
def test_knob_routes_equal_the_recorded_table(torch_gpu, monkeypatch, name):
    """tests/golden/routing_knobs.json holds the forced and special routes of three small plans (the one whose
    split-K slabs peak inside the reserved range, one with the MFMA image, tests/test_gpu_wide.py's with its
    wide streams), each as a fast-order, a reference-order and a transposed plan, under every TCSC_SLICES,
    TCSC_GEO and TCSC_COMBINE of gen_routing.py and seven values of M: path and K split, geometry (or the
    text of the refusal of TCSC_GEO=22), combine mode, the workspace of each path and what reserve(512) holds.
    Queries only, nothing is launched.  Every entry must be what it was."""
    for k in GEN_ROUTING.KNOBS + GEN_ROUTING.KNOB_ENV:
        monkeypatch.delenv(k, raising=False)  # record_knobs sets the knobs itself and leaves them cleared
    with open(GEN_ROUTING.KNOB_TABLE) as f:
        table = json.load(f)
    order = tcsc_amd.get_order()
    got = GEN_ROUTING.record_knobs(tcsc_amd, name)
    assert tcsc_amd.get_order() == order
    per_plan = len(GEN_ROUTING.KNOB_KINDS) * len(GEN_ROUTING.KNOB_SLICES) * len(GEN_ROUTING.KNOB_GEO) * \
        len(GEN_ROUTING.KNOB_COMBINE)
    assert len(got) == per_plan and set(got) <= set(table) and len(table) == per_plan * len(GEN_ROUTING.KNOB_PLANS)
    names = ("M", "path", "slices", "geometry", "combine", "workspace", "gather ws", "mfma ws", "small ws")
    for key, g in got.items():
        want = table[key]
        assert g["reserved"] == want["reserved"], f"{key}: reserve({GEN_ROUTING.KNOB_RESERVE_M})"
        assert len(g["rows"]) == len(want["rows"]) == len(GEN_ROUTING.KNOB_MS)
        for grow, wrow in zip(g["rows"], want["rows"]):
            assert grow == wrow, f"{key} M={wrow[0]}: " + ", ".join(
                f"{n} {a} (recorded {b})" for n, a, b in zip(names, grow, wrow) if a != b)


# ---- launches ---------------------------------------------------------------

def bits(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=2)
def launch_case(K, N, density, max_M):
    """W (arrays), float and integer X / B and their references for max_M rows,
    computed once: a launch of M rows is checked against the first M rows."""
    o = pyoracle.load_oracle()
    arrays = strided_arrays(K, N, density)
    Wref = pyoracle.TCSC(K, N, *arrays)
    X, B = o.uniform((max_M, K), 4100 + K), o.uniform((N,), 4101 + K)
    Xi, Bi = o.integers((max_M, K), 4102 + K), o.integers((N,), 4103 + K)
    Y64, S64 = o.f64_rows(X, Wref, B)
    Yi = o.sgemm("prelu_basic", Xi, Wref, Bi, 0.2)
    for a in (X, B, Xi, Bi, Y64, S64, Yi):
        a.setflags(write=False)
    return dict(X=X, B=B, Xi=Xi, Bi=Bi, Y64=Y64, S64=S64, Yi=Yi)


def run_sequence(torch, K, N, density, max_M, seq):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    c = launch_case(K, N, density, max_M)
    dX, dB = torch.from_numpy(c["X"]).to(dev), torch.from_numpy(c["B"]).to(dev)
    dXi, dBi = torch.from_numpy(c["Xi"]).to(dev), torch.from_numpy(c["Bi"]).to(dev)
    W = strided_w(K, N, density)
    plan = tcsc_amd.Plan(W, 0, N, 0, stream)
    plan.reserve(max_M)
    held = plan.info()["device_bytes"]
    fresh = {}
    paths = []
    for M in seq:
        paths.append(plan.launch_info(M)[0])
        assert plan.workspace(M)[0] <= plan.workspace(M)[1], f"M={M}: reserve({max_M}) does not cover it"
        Y, Yi = torch.empty((M, N), device=dev), torch.empty((M, N), device=dev)
        plan.sgemm(dX, dB, Y, M, N, "prelu_basic", 0.2, stream)
        plan.sgemm(dXi, dBi, Yi, M, N, "prelu_basic", 0.2, stream)
        torch.cuda.synchronize()
        assert plan.info()["device_bytes"] == held, f"M={M}: the plan reallocated"
        if M not in fresh:  # a plan that never saw another M, reserved at exactly this one
            q = tcsc_amd.Plan(W, 0, N, 0, stream)
            q.reserve(M)
            assert q.launch_info(M) == plan.launch_info(M)
            F, Fi = torch.empty((M, N), device=dev), torch.empty((M, N), device=dev)
            q.sgemm(dX, dB, F, M, N, "prelu_basic", 0.2, stream)
            q.sgemm(dXi, dBi, Fi, M, N, "prelu_basic", 0.2, stream)
            torch.cuda.synchronize()
            fresh[M] = (bits(F), bits(Fi))
            q.destroy()
        np.testing.assert_array_equal(bits(Y), fresh[M][0], err_msg=f"M={M} float vs fresh plan")
        np.testing.assert_array_equal(bits(Yi), fresh[M][1], err_msg=f"M={M} int vs fresh plan")
        np.testing.assert_array_equal(bits(Yi), c["Yi"][:M].view(np.uint32), err_msg=f"M={M} int vs oracle")
        ok, ratio = pyoracle.check_close(Y.cpu().numpy(), c["Y64"][:M], c["S64"][:M], 0.2)
        assert ok, f"M={M}: worst err/bound = {ratio:.3g}"
    return W, plan, paths, held, (dX, dB)


def test_launch_history_gather_plan(torch_gpu, monkeypatch):
    """K = 512, N = 4096, density 0.02, reserve(512) once, then launches of 512,
    339, 5, 200, 3, 512 rows on the same plan: the plan never reallocates, and
    every result has the bits of a fresh plan reserved at exactly that M, the
    oracle's bits on integers and the fp32 bound on floats.  Then one
    prepare_x(200) / sgemm(339) / sgemm_prepared(200): the whole launch
    overwrote the staged X^T, so the last call is TCSC_E_ARG, not stale data."""
    for k in ("TCSC_SLICES", "TCSC_PATH", "TCSC_SMALL_M"):
        monkeypatch.delenv(k, raising=False)
    torch = torch_gpu
    K, N = 512, 4096
    W, plan, paths, held, (dX, dB) = run_sequence(torch, K, N, 0.02, 512, (512, 339, 5, 200, 3, 512))
    assert paths[0] == "gather" and paths[4] == "small"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    Y = torch.full((339, N), 7.0, device=dev)
    plan.prepare_x(dX, 200, stream)
    plan.sgemm(dX, dB, Y, 339, N, "prelu_basic", 0.2, stream)
    Y.fill_(7.0)
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1"):
        plan.sgemm_prepared(dB, Y, 200, N, "prelu_basic", 0.2, stream)
    torch.cuda.synchronize()
    assert bool((Y == 7.0).all())  # nothing ran
    assert plan.info()["device_bytes"] == held
    plan.destroy()
    W.free()


def test_launch_history_mfma_plan(torch_gpu, monkeypatch):
    """The same on a plan with the MFMA image (K = 1024, N = 512, density 0.5,
    reserve(256)): 256, 64, 17, 5, 4, 130 rows cross the 128-row tiles, the
    narrow tiles of M <= 64 and the small-M path."""
    for k in ("TCSC_SLICES", "TCSC_PATH", "TCSC_SMALL_M", "TCSC_MFMA_WGS"):
        monkeypatch.delenv(k, raising=False)
    W, plan, paths, held, _ = run_sequence(torch_gpu, 1024, 512, 0.5, 256, (256, 64, 17, 5, 4, 130))
    assert paths[0] == "mfma" and paths[1] == "mfma" and paths[4] == "small", paths
    plan.destroy()
    W.free()


@pytest.mark.parametrize("K,N,density", [(512, 4096, 0.02), (1024, 512, 0.5)], ids=["slabs", "image"])
def test_pinned_split_launches_what_the_route_says(torch_gpu, monkeypatch, K, N, density):
    """TCSC_SLICES = 1, 2, 4 at plan creation, reserve(512) and launch, M = 339 and 64: the launch runs in the
    workspace the route sized (the plan never reallocates), and its rows have the bits of a launch with the
    knob unset at the largest M' <= 512 where the cost model itself takes the same path and K split (a row's
    sum depends on the split, not on how many rows run beside it; on the MFMA path, whose tiles depend on M,
    only M' = M counts).  Where no such M' exists the fp32 bound against the fp64 oracle is all there is; it
    is asked in either case."""
    torch = torch_gpu
    for k in ("TCSC_SLICES", "TCSC_PATH", "TCSC_SMALL_M", "TCSC_MFMA_WGS", "TCSC_GEO", "TCSC_COMBINE"):
        monkeypatch.delenv(k, raising=False)
    dev = torch.device("cuda:0")
    c = launch_case(K, N, density, 512)
    dX, dB = torch.from_numpy(c["X"]).to(dev), torch.from_numpy(c["B"]).to(dev)
    W = strided_w(K, N, density)

    def launch(plan, M):
        Y = torch.full((M, N), float("nan"), device=dev)
        plan.sgemm(dX, dB, Y, M, N, "prelu_basic", 0.2)
        torch.cuda.synchronize()
        return Y

    free = tcsc_amd.Plan(W)  # the cost model's own choices
    free.reserve(512)
    chosen = {M: free.launch_info(M) for M in range(1, 513)}
    same_bits = 0
    for slices in (1, 2, 4):
        monkeypatch.setenv("TCSC_SLICES", str(slices))
        plan = tcsc_amd.Plan(W)
        plan.reserve(512)
        held = plan.info()["device_bytes"]
        for M in (339, 64):
            route = plan.launch_info(M)
            assert route[0] == "mfma" or route == ("gather", slices), route
            assert plan.workspace(M)[0] <= plan.workspace(M)[1]
            Y = launch(plan, M)
            assert plan.info()["device_bytes"] == held, f"TCSC_SLICES={slices} M={M}: the plan reallocated"
            ok, ratio = pyoracle.check_close(Y.cpu().numpy(), c["Y64"][:M], c["S64"][:M], 0.2)
            print(f"TCSC_SLICES={slices} M={M}: {route}, worst err/bound {ratio:.3g}")
            assert ok, f"TCSC_SLICES={slices} M={M}: worst err/bound = {ratio:.3g}"
            twins = [m for m, r in chosen.items() if r == route and (route[0] == "gather" or m == M)]
            if twins:
                monkeypatch.delenv("TCSC_SLICES")
                m = max(twins)
                F = launch(free, m)
                monkeypatch.setenv("TCSC_SLICES", str(slices))
                rows = min(m, M)
                np.testing.assert_array_equal(bits(Y[:rows]), bits(F[:rows]),
                                              err_msg=f"TCSC_SLICES={slices} M={M} vs the cost model's M={m}")
                same_bits += 1
        plan.destroy()
    assert same_bits > 0, "no forced route met a route the cost model chose"
    free.destroy()
    W.free()


def test_graph_capture_at_a_hole(torch_gpu, monkeypatch):
    """reserve(512), then a capture of 339 rows (the M whose split-K slabs are
    the largest of any M <= 512 at this shape): the host assertion comes first,
    so a reserve that does not cover it fails before anything is captured.
    The replay has the eager bits, also after an eager launch of 200 rows on
    the same plan, and the plan never reallocates."""
    for k in ("TCSC_SLICES", "TCSC_PATH", "TCSC_SMALL_M"):
        monkeypatch.delenv(k, raising=False)
    torch = torch_gpu
    dev = torch.device("cuda:0")
    K, N, M = 512, 4096, 339
    c = launch_case(K, N, 0.02, 512)
    W = strided_w(K, N, 0.02)
    side = torch.cuda.Stream()
    plan = tcsc_amd.Plan(W, 0, N, 0, side.cuda_stream)
    plan.reserve(512)
    for m in (M, 200):
        need, reserved = plan.workspace(m)
        assert need <= reserved, f"reserve(512) holds {reserved} bytes, M={m} needs {need}"
    held = plan.info()["device_bytes"]
    X, B = torch.from_numpy(c["X"]).to(dev), torch.from_numpy(c["B"]).to(dev)
    Ye = torch.empty((M, N), device=dev)
    with torch.cuda.stream(side):
        plan.sgemm(X, B, Ye, M, N, "prelu_basic", 0.2, side.cuda_stream)
    side.synchronize()
    eager = bits(Ye).copy()
    ok, ratio = pyoracle.check_close(Ye.cpu().numpy(), c["Y64"][:M], c["S64"][:M], 0.2)
    assert ok, f"worst err/bound = {ratio:.3g}"
    Yg = torch.full((M, N), float("nan"), device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.sgemm(X, B, Yg, M, N, "prelu_basic", 0.2, torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(Yg), eager)
    Y2 = torch.empty((200, N), device=dev)
    with torch.cuda.stream(side):
        plan.sgemm(X, B, Y2, 200, N, "prelu_basic", 0.2, side.cuda_stream)
    side.synchronize()
    assert plan.info()["device_bytes"] == held
    Yg.fill_(float("nan"))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(Yg), eager)
    assert plan.info()["device_bytes"] == held
    del g
    plan.destroy()
    W.free()
