"""Saving and loading packed plans on the device: image -> packed plan (k_w2_check), image -> TCSC
(k_w2_unpack), the file layer and PackedTernaryLinear's state_dict.

No tolerance anywhere: every comparison is of bytes or bits.  Yardsticks, never the loaded plan itself: the plan
tcsc_gpu_plan_create_packed builds from the TCSC arrays, tcsc_from_dense's arrays of the dense matrix, and the
host-only packer (itself pinned to a numpy restatement of the layout by tests/test_packed_io_api.py).

The grid is the smallest at which a kernel can go wrong: K around the 16-k dword and the 256-k block and over several
blocks, N around the 16-column tile and over three tiles, W all zero, all +1, all -1 and two thirds full."""
import io

import numpy as np
import pytest

import tcsc_amd
from packed_io_cases import CORRUPTIONS, FILLS, KS, NS, SHARD, poke, weights

pytestmark = pytest.mark.gpu

KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_DECODE", "TCSC_W2GEMM", "TCSC_ORDER")
GEMM_SHAPES = ((300, 33), (1025, 17), (2177, 513))
MS = (1, 16, 17, 70)
MAXM = 70


@pytest.fixture(scope="module")
def gpu():
    tcsc_amd.build()
    tcsc_amd.require_gpu()
    tcsc_amd.set_num_shards(0)
    import torch

    return torch


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    tcsc_amd.set_order("fast")


def dev(torch):
    return torch.device("cuda:0")


def image_of(torch, plan):
    img = plan.w2_image()
    torch.cuda.synchronize()
    assert img.dtype == torch.uint8 and img.is_cuda and img.is_contiguous()
    return img


def assert_same_arrays(got, want, what):
    for g, w, name in zip(got, want, ("col_start_pos", "col_start_neg", "row_index_pos", "row_index_neg")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}: {name}"


_gemm_cases = {}


def gemm_case(torch, K, N):
    """W, a full-range int8 X of MAXM rows, a float bias and float row scales on the device: made once per shape."""
    if (K, N) not in _gemm_cases:
        rng = np.random.default_rng(19500 + K + N)
        Xq = rng.integers(-128, 128, (MAXM, K), dtype=np.int64).astype(np.int8)
        Xq[2, :] = -128
        B = rng.uniform(-1, 1, N).astype(np.float32)
        s = (rng.uniform(0, 1, MAXM) * 0.05 + 1e-3).astype(np.float32)
        _gemm_cases[(K, N)] = dict(Wd=weights(K, N, "0.67"), Xq=torch.from_numpy(Xq).to(dev(torch)),
                                   B=torch.from_numpy(B).to(dev(torch)), s=torch.from_numpy(s).to(dev(torch)))
    return _gemm_cases[(K, N)]


# ---- 1. image -> packed plan ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_round_trip_over_the_grid(gpu, K):
    torch = gpu
    for N in NS:
        for fill in FILLS:
            what = f"K={K} N={N} {fill}"
            W = tcsc_amd.TcscMatrix.from_dense(weights(K, N, fill))
            first = tcsc_amd.Plan.packed(W)
            img = image_of(torch, first)
            assert img.numel() == tcsc_amd.w2_image_bytes(K, N), what
            assert np.array_equal(img.cpu().numpy(), tcsc_amd.w2_pack_host(W)), what
            want = first.info()
            assert want["nnz"] == W.nnz and want["device_bytes"] == img.numel(), what
            for source in (img, img.cpu().numpy(), img.data_ptr()):  # device tensor, host array, device pointer
                loaded = tcsc_amd.Plan.packed_from_image(source, K, N)
                assert loaded.is_packed and loaded.has_w2 and not loaded.has_i8, what
                assert loaded.info() == want, (what, loaded.info(), want)
                assert torch.equal(image_of(torch, loaded), img), what
                for M in (1, 16, 17, 300):
                    assert loaded.launch_info_i8(M) == first.launch_info_i8(M), (what, M)
                    assert loaded.workspace(M) == first.workspace(M), (what, M)
                loaded.destroy()
            first.destroy()
            W.free()


def test_an_image_of_more_tiles_than_the_check_kernel_has_workgroups(gpu):
    """k_w2_check runs at most 1024 workgroups of 256 dwords: from 1025 tiles on its threads stride over the image.
    9 k blocks x 129 column tiles = 1161 tiles, with a K tail and a column tail."""
    torch = gpu
    K, N = 2049, 2050
    assert tcsc_amd.w2_image_bytes(K, N) // 1024 == 1161
    Wd = weights(K, N, "0.67")
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    first = tcsc_amd.Plan.packed(W)
    img = image_of(torch, first)
    loaded = tcsc_amd.Plan.packed_from_image(img, K, N)
    assert loaded.info() == first.info()
    assert (loaded.info()["n_pos"], loaded.info()["n_neg"]) == (int((Wd == 1).sum()), int((Wd == -1).sum()))
    assert torch.equal(image_of(torch, loaded), img)
    assert_same_arrays(tcsc_amd.w2_to_tcsc(img, K, N), W.arrays(), "strided check")
    for p in (first, loaded):
        p.destroy()
    W.free()


def test_a_column_shard_reloads_with_its_label(gpu):
    torch = gpu
    K, (c0, c1) = 300, SHARD
    W = tcsc_amd.TcscMatrix.from_dense(weights(K, 33, "0.67"))
    first = tcsc_amd.Plan.packed(W, c0, c1)
    img = image_of(torch, first)
    assert np.array_equal(img.cpu().numpy(), tcsc_amd.w2_pack_host(W, c0, c1))
    loaded = tcsc_amd.Plan.packed_from_image(img, K, c1 - c0, col_begin=c0)
    assert loaded.info() == first.info() and loaded.info()["col_begin"] == c0
    assert torch.equal(image_of(torch, loaded), img)
    # the plan owns a copy: the caller's image may go
    img.fill_(0xFF)
    torch.cuda.synchronize()
    assert np.array_equal(image_of(torch, loaded).cpu().numpy(), tcsc_amd.w2_pack_host(W, c0, c1))
    for p in (first, loaded):
        p.destroy()
    W.free()


def test_a_loaded_plan_refuses_what_a_packed_plan_refuses(gpu):
    torch = gpu
    K, N = 64, 32
    W = tcsc_amd.TcscMatrix.from_dense(weights(K, N, "0.67"))
    loaded = tcsc_amd.Plan.packed_from_image(tcsc_amd.w2_pack_host(W), K, N)
    X = torch.zeros((4, K), device=dev(torch))
    B = torch.zeros(N, device=dev(torch))
    Y = torch.zeros((4, N), device=dev(torch))
    with pytest.raises(tcsc_amd.TcscError, match="packed plan"):
        loaded.sgemm(X, B, Y, 4, N)
    with pytest.raises(tcsc_amd.TcscError, match="packed plan"):
        loaded.launch_info(4)
    assert loaded.enable_i8() is False and loaded.enable_w2() is True
    loaded.destroy()
    W.free()


@pytest.mark.parametrize("K,N", GEMM_SHAPES)
def test_sgemm_i8_has_the_same_bits_on_the_loaded_plan(gpu, K, N):
    torch = gpu
    c = gemm_case(torch, K, N)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    first = tcsc_amd.Plan.packed(W)
    loaded = tcsc_amd.Plan.packed_from_image(image_of(torch, first), K, N)
    ldy = N + 3
    for M in MS:
        for variant in ("basic", "prelu_basic"):
            for scale in (None, c["s"][:M]):
                out = []
                for plan in (first, loaded):
                    Y = torch.full((M, ldy), 7.0, device=dev(torch))
                    plan.sgemm_i8(c["Xq"][:M], scale, c["B"], Y, M, ldy, variant, 0.25)
                    torch.cuda.synchronize()
                    out.append(Y)
                what = f"M={M} {variant} scale={'none' if scale is None else 'float'}"
                assert not torch.isnan(out[0]).any() and torch.all(out[0][:, N:] == 7.0), what
                assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), what
    for p in (first, loaded):
        p.destroy()
    W.free()


def test_a_loaded_plan_reserves_and_is_captured_as_the_original(gpu):
    torch = gpu
    K, N = 2177, 513
    c = gemm_case(torch, K, N)
    W = tcsc_amd.TcscMatrix.from_dense(c["Wd"])
    first = tcsc_amd.Plan.packed(W)
    loaded = tcsc_amd.Plan.packed_from_image(image_of(torch, first), K, N)
    for p in (first, loaded):
        p.reserve(MAXM)
    assert loaded.info() == first.info() and loaded.info()["device_bytes"] > tcsc_amd.w2_image_bytes(K, N)
    held = loaded.info()["device_bytes"]
    side = torch.cuda.Stream()
    for M in (16, MAXM):
        Qg = torch.zeros((M, K), dtype=torch.int8, device=dev(torch))
        Yg = torch.empty((M, N), device=dev(torch))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            loaded.sgemm_i8(Qg, c["s"][:M], c["B"], Yg, M, N, "prelu_basic", 0.2, torch.cuda.current_stream().cuda_stream)
        for r0 in (0, MAXM - M):
            Qg.copy_(c["Xq"][r0:r0 + M] if r0 == 0 else -c["Xq"][r0:r0 + M].clamp(min=-127))
            Yg.fill_(float("nan"))
            want = torch.empty((M, N), device=dev(torch))
            first.sgemm_i8(Qg, c["s"][:M], c["B"], want, M, N, "prelu_basic", 0.2)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert not torch.isnan(Yg).any() and torch.equal(Yg.view(torch.int32), want.view(torch.int32)), (M, r0)
        del g
        assert loaded.info()["device_bytes"] == held, M
    for p in (first, loaded):
        p.destroy()
    W.free()


@pytest.mark.parametrize("name,K,N,where,word", CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_the_kernel_refuses_invalid_images(gpu, name, K, N, where, word):
    torch = gpu
    W = tcsc_amd.TcscMatrix.from_dense(weights(K, N, "0.67"))
    good = tcsc_amd.w2_pack_host(W)
    W.free()
    bad = torch.from_numpy(poke(good, where[0], where[1], K, where[2])).to(dev(torch))
    other = "padding" if word == "code 3" else "code 3"
    for call, who in ((lambda: tcsc_amd.Plan.packed_from_image(bad, K, N), "tcsc_gpu_plan_create_packed_image_device"),
                      (lambda: tcsc_amd.Plan.packed_from_image(bad.cpu().numpy(), K, N),
                       "tcsc_gpu_plan_create_packed_image"),
                      (lambda: tcsc_amd.w2_to_tcsc(bad, K, N), "tcsc_gpu_w2_to_tcsc")):
        with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*" + who + ": invalid image.*" + word):
            call()
        assert other not in tcsc_amd.last_error()
    # no plan came out of the C call either
    import ctypes as C

    h = C.c_void_p(1)
    rc = tcsc_amd.lib().tcsc_gpu_plan_create_packed_image_device(C.c_void_p(bad.data_ptr()), bad.numel(), K, N, 0, 0,
                                                                 None, C.byref(h))
    assert rc == 1 and not h.value
    tcsc_amd.Plan.packed_from_image(torch.from_numpy(good).to(dev(torch)), K, N).destroy()  # the good one loads


def test_both_faults_are_named_when_both_are_there(gpu):
    torch = gpu
    K, N = 300, 17
    W = tcsc_amd.TcscMatrix.from_dense(weights(K, N, "0.67"))
    bad = poke(poke(tcsc_amd.w2_pack_host(W), 7, 3, K, 3), 300, 0, K, 2)
    W.free()
    with pytest.raises(tcsc_amd.TcscError, match="code 3.*padding"):
        tcsc_amd.Plan.packed_from_image(torch.from_numpy(bad).to(dev(torch)), K, N)


# ---- 2. image -> TCSC -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_w2_to_tcsc_over_the_grid(gpu, K):
    torch = gpu
    for N in NS:
        for fill in FILLS:
            what = f"K={K} N={N} {fill}"
            Wd = weights(K, N, fill)
            W = tcsc_amd.TcscMatrix.from_dense(Wd)
            host_img = tcsc_amd.w2_pack_host(W)
            img = torch.from_numpy(host_img).to(dev(torch))
            # the counts-only call on its own: col_start and the totals, nothing else touched
            import ctypes as C

            csp = torch.full((N + 1,), -1, dtype=torch.int32, device=dev(torch))
            csn = torch.full((N + 1,), -1, dtype=torch.int32, device=dev(torch))
            p, q = C.c_int(-1), C.c_int(-1)
            rc = tcsc_amd.lib().tcsc_gpu_w2_to_tcsc(C.c_void_p(img.data_ptr()), img.numel(), K, N,
                                                    C.c_void_p(csp.data_ptr()), C.c_void_p(csn.data_ptr()), None, None,
                                                    C.byref(p), C.byref(q), None)
            want = W.arrays()
            assert rc == 0 and (p.value, q.value) == (want[2].size, want[3].size), what
            assert_same_arrays((csp, csn), want[:2], what + " counts call")
            got = tcsc_amd.w2_to_tcsc(img, K, N)
            assert_same_arrays(got, want, what)
            back = tcsc_amd.w2_unpack_host(host_img, K, N)
            assert_same_arrays(got, back.arrays(), what + " vs host")
            back.free()
            W.free()


def test_w2_to_tcsc_of_a_column_shard(gpu):
    torch = gpu
    K, (c0, c1) = 1025, SHARD
    Wd = weights(K, 33, "0.67")
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    plan = tcsc_amd.Plan.packed(W, c0, c1)
    got = tcsc_amd.w2_to_tcsc(image_of(torch, plan), K, c1 - c0)
    want = tcsc_amd.TcscMatrix.from_dense(np.ascontiguousarray(Wd[:, c0:c1]))
    assert_same_arrays(got, want.arrays(), "shard")
    plan.destroy()
    for m in (W, want):
        m.free()


def test_an_unpacked_image_builds_an_ordinary_plan_with_the_same_sgemm_bits(gpu):
    torch = gpu
    M, K, N = 8, 300, 33
    W = tcsc_amd.TcscMatrix.from_dense(weights(K, N, "0.67"))
    packed = tcsc_amd.Plan.packed(W)
    csp, csn, rip, rin = tcsc_amd.w2_to_tcsc(image_of(torch, packed), K, N)
    rebuilt = tcsc_amd.Plan.from_device(K, N, csp, csn, rip, rin)
    direct = tcsc_amd.Plan(W)
    assert rebuilt.info() == direct.info()
    rng = np.random.default_rng(19700)
    X = torch.from_numpy(rng.integers(-8, 9, (M, K)).astype(np.float32)).to(dev(torch))
    B = torch.from_numpy(rng.integers(-8, 9, N).astype(np.float32)).to(dev(torch))
    out = []
    for plan in (direct, rebuilt):
        Y = torch.full((M, N), float("nan"), device=dev(torch))
        plan.sgemm(X, B, Y, M, N, "prelu_basic", 0.25)
        torch.cuda.synchronize()
        out.append(Y)
    assert not torch.isnan(out[0]).any() and torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
    for p in (packed, rebuilt, direct):
        p.destroy()
    W.free()


# ---- 3. files and the torch layer -------------------------------------------------------------------------------------

def test_save_packed_and_load_packed_round_trip(gpu, tmp_path):
    torch = gpu
    K, (c0, c1) = 300, SHARD
    W = tcsc_amd.TcscMatrix.from_dense(weights(K, 33, "0.67"))
    first = tcsc_amd.Plan.packed(W, c0, c1)
    path = str(tmp_path / "layer.npz")
    tcsc_amd.save_packed(first, path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["col_begin", "cols", "image", "rows", "version"]
        assert z["image"].dtype == np.uint8 and (int(z["rows"]), int(z["cols"]), int(z["col_begin"])) == (K, c1 - c0, c0)
    loaded = tcsc_amd.load_packed(path)
    assert loaded.info() == first.info()
    assert torch.equal(image_of(torch, loaded), image_of(torch, first))
    for p in (first, loaded):
        p.destroy()
    W.free()


def test_packed_ternary_linear_state_dict_round_trip(gpu):
    torch = gpu
    from tcsc_amd.nn import PackedTernaryLinear

    K, N = 300, 33
    Wd = weights(K, N, "0.67")
    rng = np.random.default_rng(19800)
    layer = PackedTernaryLinear(Wd, bias=rng.uniform(-1, 1, N).astype(np.float32), a=0.2)
    sd = layer.state_dict()
    assert set(sd) == {"bias", "w2"}
    assert sd["w2"].dtype == torch.uint8 and sd["w2"].numel() == tcsc_amd.w2_image_bytes(K, N)
    assert "w2" not in dict(layer.named_buffers())           # the layer does not hold the image twice
    assert sd["w2"].data_ptr() != layer.state_dict()["w2"].data_ptr()  # a fresh copy per call
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    sd2 = torch.load(f, weights_only=True)
    assert set(sd2) == {"bias", "w2"}

    fresh = PackedTernaryLinear.empty(K, N, a=0.2)
    x3 = torch.from_numpy(rng.uniform(-2, 2, (3, K)).astype(np.float32)).to(dev(torch))
    x40 = torch.from_numpy(rng.uniform(-2, 2, (40, K)).astype(np.float32)).to(dev(torch))
    with pytest.raises(tcsc_amd.TcscError, match="empty"):
        fresh(x3)
    with pytest.raises(tcsc_amd.TcscError, match="empty"):
        fresh.reserve(8)
    with pytest.raises(tcsc_amd.TcscError, match="empty"):
        fresh.state_dict()
    # a missing key and an image of another shape: refused, the layer stays empty
    with pytest.raises(tcsc_amd.TcscError, match="missing key 'w2'"):
        fresh.load_state_dict({"bias": sd2["bias"]})
    with pytest.raises(tcsc_amd.TcscError, match="missing key 'bias'"):
        fresh.load_state_dict({"w2": sd2["w2"]}, strict=False)
    with pytest.raises(tcsc_amd.TcscError, match="needs"):
        fresh.load_state_dict({"bias": sd2["bias"], "w2": sd2["w2"][:-1024]})
    with pytest.raises(tcsc_amd.TcscError, match="bias"):
        fresh.load_state_dict({"bias": sd2["bias"][:-1], "w2": sd2["w2"]})
    assert fresh.nnz == 0 and fresh.plan is None
    with pytest.raises(RuntimeError, match="[Uu]nexpected"):  # torch's own strictness still sees other keys
        fresh.load_state_dict({"bias": sd2["bias"], "w2": sd2["w2"], "other": sd2["bias"]})

    fresh = PackedTernaryLinear.empty(K, N, a=0.2)
    result = fresh.load_state_dict(sd2)
    assert not result.missing_keys and not result.unexpected_keys
    assert fresh.nnz == layer.nnz == np.count_nonzero(Wd)
    assert fresh.plan.info() == layer.plan.info()
    for x in (x3, x40):
        want, got = layer(x), fresh(x)
        torch.cuda.synchronize()
        assert not torch.isnan(want).any() and torch.equal(want.view(torch.int32), got.view(torch.int32)), x.shape
    # a load that replaces a plan: the old plan and its reserve are gone, the new one serves
    fresh.reserve(40)
    assert fresh.plan.workspace(40)[1] > 0
    fresh.load_state_dict({k: v.cpu() for k, v in sd2.items()})  # a CPU state_dict (map_location="cpu") loads too
    assert fresh.plan.workspace(40)[1] == 0
    got = fresh(x40)
    torch.cuda.synchronize()
    assert torch.equal(layer(x40).view(torch.int32), got.view(torch.int32))
