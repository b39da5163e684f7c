"""Saving and loading packed plans, the part that needs no GPU: the new functions are declared, listed,
exported and bound; what they can refuse on the host they refuse with TCSC_E_ARG and the call's name before any HIP
call; the host-only packer and unpacker against a numpy restatement of the header's layout and against
tcsc_from_dense; invalid images and invalid files.  What the device side computes is tests/test_gpu_packed_io.py's."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import tcsc_amd
from conftest import ROOT
from packed_io_cases import CORRUPTIONS, FILLS, KS, NS, SHARD, layout_image, poke, weights

NEW_SYMBOLS = ("tcsc_gpu_plan_create_packed_image", "tcsc_gpu_plan_create_packed_image_device", "tcsc_gpu_w2_to_tcsc",
               "tcsc_gpu_w2_from_tcsc_host", "tcsc_gpu_w2_to_tcsc_host")
E_ARG = 1


@pytest.fixture(scope="module")
def built_lib():
    tcsc_amd.build()
    return tcsc_amd.lib()


def assert_same_arrays(got, want, what):
    for g, w, name in zip(got, want, ("col_start_pos", "col_start_neg", "row_index_pos", "row_index_neg")):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}: {name}"


def test_symbols_are_declared_listed_exported_and_bind(built_lib):
    header = open(os.path.join(ROOT, "include", "tcsc_gpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", tcsc_amd.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int\s+|tcsc_t\s*\*)" + name + r"\s*\(", header), f"{name} not declared in tcsc_gpu.h"
        assert name in tcsc_amd.EXPORTED_SYMBOLS, name
        assert name in exported, name
        assert getattr(built_lib, name).argtypes is not None, name
    assert (built_lib.tcsc_gpu_plan_create_packed_image.argtypes ==
            built_lib.tcsc_gpu_plan_create_packed_image_device.argtypes)


def test_arguments_are_refused_on_the_host_before_any_hip_call(built_lib):
    """NULL arguments, a wrong byte count, rows = 0, rows = 2^22, cols = 0, a negative col_begin and a reference-order
    request: TCSC_E_ARG (a device touch would be TCSC_E_HIP or TCSC_E_NODEV where there is no device) and a message
    that names the call; *out stays NULL.  The image pointers are never read: refused first."""
    img = np.full(1024, 0x55, np.uint8)  # the image of a 4 x 4 zero matrix
    p = C.c_void_p(img.ctypes.data)
    one = C.c_void_p(16)
    for name in ("tcsc_gpu_plan_create_packed_image", "tcsc_gpu_plan_create_packed_image_device"):
        f = getattr(built_lib, name)
        h = C.c_void_p(1)  # the call must reset it

        def refused(rc, word=None):
            assert rc == E_ARG, (name, rc, tcsc_amd.last_error())
            assert tcsc_amd.last_error().startswith(name + ":"), tcsc_amd.last_error()
            assert word is None or word in tcsc_amd.last_error(), tcsc_amd.last_error()
            assert not h.value

        refused(f(None, 1024, 4, 4, 0, 0, None, C.byref(h)), "NULL")
        assert f(p, 1024, 4, 4, 0, 0, None, None) == E_ARG and name in tcsc_amd.last_error()
        refused(f(p, 1023, 4, 4, 0, 0, None, C.byref(h)), "bytes")
        refused(f(p, 2048, 4, 4, 0, 0, None, C.byref(h)), "bytes")
        refused(f(p, 1024, 0, 4, 0, 0, None, C.byref(h)), "K")
        refused(f(p, (1 << 14) * 1024, 1 << 22, 4, 0, 0, None, C.byref(h)), "K")
        refused(f(p, 1024, 4, 0, 0, 0, None, C.byref(h)), "cols")
        refused(f(p, 1024, 4, 4, -1, 0, None, C.byref(h)), "col_begin")
        tcsc_amd.set_order("reference")
        try:
            refused(f(p, 1024, 4, 4, 0, 0, None, C.byref(h)), "reference")
            with pytest.raises(tcsc_amd.TcscError, match="reference"):
                tcsc_amd.Plan.packed_from_image(img, 4, 4)
        finally:
            tcsc_amd.set_order("fast")
    f, name = built_lib.tcsc_gpu_w2_to_tcsc, "tcsc_gpu_w2_to_tcsc"
    n = C.c_int(-7)
    for rc in (f(None, 1024, 4, 4, one, one, None, None, C.byref(n), C.byref(n), None),
               f(one, 1024, 4, 4, None, one, None, None, C.byref(n), C.byref(n), None),
               f(one, 1024, 4, 4, one, one, None, None, None, C.byref(n), None),
               f(one, 1000, 4, 4, one, one, None, None, C.byref(n), C.byref(n), None),
               f(one, 1024, 0, 4, one, one, None, None, C.byref(n), C.byref(n), None),
               f(one, (1 << 14) * 1024, 1 << 22, 4, one, one, None, None, C.byref(n), C.byref(n), None),
               f(one, 1024, 4, 0, one, one, None, None, C.byref(n), C.byref(n), None)):
        assert rc == E_ARG and tcsc_amd.last_error().startswith(name + ":"), (rc, tcsc_amd.last_error())
    assert n.value == -7


def test_host_functions_refuse_bad_arguments(built_lib):
    W = tcsc_amd.TcscMatrix.from_dense(np.eye(4, dtype=np.float32))
    img = np.zeros(1024, np.uint8)
    p = C.c_void_p(img.ctypes.data)
    f, name = built_lib.tcsc_gpu_w2_from_tcsc_host, "tcsc_gpu_w2_from_tcsc_host"
    for rc in (f(None, 0, 4, p, 1024), f(W.ptr, 0, 4, None, 1024), f(W.ptr, 0, 4, p, 1023), f(W.ptr, 2, 5, p, 1024),
               f(W.ptr, 3, 2, p, 1024), f(W.ptr, 2, 2, p, 0)):
        assert rc == E_ARG and tcsc_amd.last_error().startswith(name + ":"), (rc, tcsc_amd.last_error())
    g, name = built_lib.tcsc_gpu_w2_to_tcsc_host, "tcsc_gpu_w2_to_tcsc_host"
    for ptr in (g(None, 1024, 4, 4), g(p, 1023, 4, 4), g(p, 1024, 0, 4), g(p, (1 << 14) * 1024, 1 << 22, 4),
                g(p, 1024, 4, 0)):
        assert not ptr and tcsc_amd.last_error().startswith(name + ":"), tcsc_amd.last_error()
    # a row outside [0, K) and a col_start that runs backwards
    bad = tcsc_amd.TcscMatrix.from_arrays(4, 2, [0, 1, 2], [0, 0, 0], [1, 4], [])
    with pytest.raises(tcsc_amd.TcscError, match="row index"):
        tcsc_amd.w2_pack_host(bad)
    bad.free()
    bad = tcsc_amd.TcscMatrix.from_arrays(4, 2, [0, 2, 1], [0, 0, 0], [1, 2], [])
    with pytest.raises(tcsc_amd.TcscError, match="col_start"):
        tcsc_amd.w2_pack_host(bad)
    bad.free()
    W.free()
    with pytest.raises(tcsc_amd.TcscError, match="freed"):
        tcsc_amd.w2_pack_host(W)
    with pytest.raises(tcsc_amd.TcscError, match="uint8"):
        tcsc_amd.w2_unpack_host(np.zeros(1024, np.int8), 4, 4)


@pytest.mark.parametrize("K", KS)
def test_host_pack_and_unpack_over_the_grid(built_lib, K):
    for N in NS:
        for fill in FILLS:
            what = f"K={K} N={N} {fill}"
            Wd = weights(K, N, fill)
            W = tcsc_amd.TcscMatrix.from_dense(Wd)
            img = tcsc_amd.w2_pack_host(W)
            assert img.dtype == np.uint8 and img.size == tcsc_amd.w2_image_bytes(K, N), what
            assert np.array_equal(img, layout_image(Wd)), what
            back = tcsc_amd.w2_unpack_host(img, K, N)
            assert (back.rows, back.cols) == (K, N), what
            assert_same_arrays(back.arrays(), W.arrays(), what)
            back.free()
            W.free()


@pytest.mark.parametrize("K", KS)
def test_a_column_shard_unpacks_to_the_slice_from_zero(built_lib, K):
    c0, c1 = SHARD
    Wd = weights(K, 33, "0.67")
    W = tcsc_amd.TcscMatrix.from_dense(Wd)
    img = tcsc_amd.w2_pack_host(W, c0, c1)
    assert np.array_equal(img, layout_image(Wd[:, c0:c1]))
    back = tcsc_amd.w2_unpack_host(img, K, c1 - c0)
    want = tcsc_amd.TcscMatrix.from_dense(np.ascontiguousarray(Wd[:, c0:c1]))
    assert back.arrays()[0][0] == 0 and back.arrays()[1][0] == 0
    assert_same_arrays(back.arrays(), want.arrays(), f"K={K} shard")
    for m in (back, want, W):
        m.free()


def test_unsorted_columns_and_cancelling_pairs_give_the_summed_matrix(built_lib):
    K, N = 300, 17
    Wd = weights(K, N, "0.67")
    Wd[[10, 299], 4] = 0.0  # where the pairs go
    csp, csn, rip, rin = tcsc_amd.TcscMatrix.from_dense(Wd).arrays()
    # a +1 and a -1 at (10, 4) and at (299, 4): both lists of column 4 grow by two, every later offset moves
    def with_pairs(cs, ri):
        at = cs[5]
        return np.concatenate([cs[:5], cs[5:] + 2]), np.concatenate([ri[:at], [299, 10], ri[at:]])

    csp2, rip2 = with_pairs(csp, rip)
    csn2, rin2 = with_pairs(csn, rin)
    rng = np.random.default_rng(5)
    for j in range(N):  # and every column out of order
        rng.shuffle(rip2[csp2[j]:csp2[j + 1]])
        rng.shuffle(rin2[csn2[j]:csn2[j + 1]])
    W2 = tcsc_amd.TcscMatrix.from_arrays(K, N, csp2, csn2, rip2, rin2)
    assert W2.nnz == np.count_nonzero(Wd) + 4
    img = tcsc_amd.w2_pack_host(W2)
    assert np.array_equal(img, layout_image(Wd))
    W2.free()


def test_a_duplicated_index_is_refused(built_lib):
    K, N = 300, 17
    csp, csn, rip, rin = tcsc_amd.TcscMatrix.from_dense(weights(K, N, "0.67")).arrays()
    rip = rip.copy()
    rip[csp[3] + 1] = rip[csp[3]]  # column 3 names one row twice: weight +2
    assert csp[4] - csp[3] >= 2
    W = tcsc_amd.TcscMatrix.from_arrays(K, N, csp, csn, rip, rin)
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\).*tcsc_gpu_w2_from_tcsc_host.*not ternary"):
        tcsc_amd.w2_pack_host(W)
    W.free()


@pytest.mark.parametrize("name,K,N,where,word", CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_invalid_images_are_refused_on_the_host(built_lib, name, K, N, where, word):
    W = tcsc_amd.TcscMatrix.from_dense(weights(K, N, "0.67"))
    good = tcsc_amd.w2_pack_host(W)
    W.free()
    tcsc_amd.w2_unpack_host(good, K, N).free()
    bad = poke(good, where[0], where[1], K, where[2])
    assert np.count_nonzero(bad != good) == 1
    with pytest.raises(tcsc_amd.TcscError, match="tcsc_gpu_w2_to_tcsc_host: invalid image.*" + word):
        tcsc_amd.w2_unpack_host(bad, K, N)
    other = "padding" if word == "code 3" else "code 3"
    assert other not in tcsc_amd.last_error()


def _npz(path, **over):
    d = dict(image=np.full(1024, 0x55, np.uint8), rows=np.int64(4), cols=np.int64(4), col_begin=np.int64(0),
             version=np.int64(tcsc_amd.PACKED_FORMAT_VERSION))
    d.update(over)
    np.savez(path, **{k: v for k, v in d.items() if v is not None})
    return str(path)


def test_load_packed_refuses_bad_files_before_the_library_is_called(built_lib, tmp_path, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(tcsc_amd, "lib", no_library)
    cases = (("version", dict(version=np.int64(tcsc_amd.PACKED_FORMAT_VERSION + 1)), "version"),
             ("dtype", dict(image=np.full(1024, 0x55, np.int8)), "uint8"),
             ("short", dict(image=np.full(1023, 0x55, np.uint8)), "1023 bytes"),
             ("shape", dict(rows=np.int64(257)), "need 2048"),
             ("nokey", dict(cols=None), "missing cols"))
    for name, over, word in cases:
        with pytest.raises(tcsc_amd.TcscError, match=word):
            tcsc_amd.load_packed(_npz(tmp_path / (name + ".npz"), **over))
    # a pickled object is never loaded
    np.savez(tmp_path / "pickle.npz", image=np.array([{"a": 1}], dtype=object), rows=4, cols=4, col_begin=0, version=1)
    with pytest.raises(ValueError, match="[Pp]ickle"):
        tcsc_amd.load_packed(str(tmp_path / "pickle.npz"))


def test_python_surface():
    assert callable(tcsc_amd.Plan.packed_from_image) and callable(tcsc_amd.Plan.w2_image)
    sig = inspect.signature(tcsc_amd.Plan.packed_from_image)
    assert list(sig.parameters) == ["image", "rows", "cols", "col_begin", "device", "stream"]
    assert list(inspect.signature(tcsc_amd.w2_to_tcsc).parameters) == ["image", "rows", "cols", "stream"]
    assert list(inspect.signature(tcsc_amd.w2_pack_host).parameters) == ["W", "col_begin", "col_end"]
    assert list(inspect.signature(tcsc_amd.w2_unpack_host).parameters) == ["image", "rows", "cols"]
    assert list(inspect.signature(tcsc_amd.save_packed).parameters) == ["plan", "path"]
    assert list(inspect.signature(tcsc_amd.load_packed).parameters) == ["path", "device", "stream"]
    with pytest.raises(tcsc_amd.TcscError, match="uint8"):
        tcsc_amd.Plan.packed_from_image(np.zeros(1024, np.int32), 4, 4)
    import tcsc_amd.nn as nn

    src = inspect.getsource(nn)
    assert "def empty(cls, in_features" in src and "_save_to_state_dict" in src and "_load_from_state_dict" in src


def test_a_plan_cannot_be_loaded_without_a_device(built_lib, tmp_path):
    if tcsc_amd.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(tcsc_amd.TcscError, match=r"status [24]\)"):
        tcsc_amd.Plan.packed_from_image(np.full(1024, 0x55, np.uint8), 4, 4)
    with pytest.raises(tcsc_amd.TcscError, match=r"status [24]\)"):
        tcsc_amd.load_packed(_npz(tmp_path / "good.npz"))
