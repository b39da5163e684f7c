"""Python mirror of the TCSC drop-in API (ctypes over libtcsc_amd.so).

Names and argument order follow the reference's C API (sparse/tcsc.h:19-48,
argument order (M, N, K) handled internally); numpy arrays stand in for
``dense_t`` and :class:`TcscMatrix` owns a ``tcsc_t*`` created by the
library's ``tcsc_from_dense``.  The device API of include/tcsc_gpu.h is
exposed through :class:`Plan`, which takes raw device pointers (ints) or
torch tensors.

There is no CPU fallback: importing works without a GPU (so the ABI can be
checked on a build host), but every compute call needs the gfx950 HIP
library and a visible device, and raises :class:`TcscError` otherwise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# TCSC_AMD_LIB points at an alternative build (e.g. the timing-only ablation
# builds of `make ablation`); default: the in-tree library.
LIB_PATH = os.environ.get("TCSC_AMD_LIB") or os.path.join(PKG_DIR, "lib", "libtcsc_amd.so")

VARIANTS = ("basic", "optimized", "prelu_basic", "prelu_separate", "prelu_onthego")
VARIANT_ID = {v: i for i, v in enumerate(VARIANTS)}
# SparseGEMM.h's sparseGEMM<float> (include/tcsc_gpu.h TCSC_VARIANT_SPARSE_GEMM):
# bias last, no activation; accepted by the device API (Plan.sgemm)
VARIANT_ID["sparse_gemm"] = 5
PRELU_VARIANTS = frozenset(VARIANTS[2:])

# every symbol include/*.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = (
    # include/sparse/tcsc.h
    "tcsc_from_dense", "tcsc_sgemm_basic", "tcsc_sgemm_optimized", "tcsc_sgemm_prelu_basic",
    "tcsc_sgemm_prelu_optimized_separate", "tcsc_sgemm_prelu_optimized_onthego", "tcsc_free",
    # include/dense/dense.h
    "dense_random", "init_rand_dense", "init_rand_sparse", "compare", "gemm_basic", "gemm_prelu_basic",
    "tcsc_set_seed",
    # include/tcsc_gpu.h
    "tcsc_gpu_device_count", "tcsc_gpu_plan_create", "tcsc_gpu_plan_create_device", "tcsc_gpu_plan_get_info",
    "tcsc_gpu_plan_reserve", "tcsc_gpu_plan_destroy", "tcsc_gpu_sgemm", "tcsc_gpu_prepare_x",
    "tcsc_gpu_sgemm_prepared", "tcsc_gpu_from_dense", "tcsc_gpu_dense_sgemm", "tcsc_gpu_last_error",
    "tcsc_gpu_cache_clear", "tcsc_gpu_num_shards", "tcsc_gpu_set_num_shards", "tcsc_gpu_set_order",
    "tcsc_gpu_get_order", "tcsc_gpu_launch_info", "tcsc_gpu_launch_combine", "tcsc_gpu_build_flags",
    "tcsc_gpu_plan_workspace", "tcsc_gpu_transpose_index", "tcsc_gpu_plan_create_transposed",
    "tcsc_gpu_plan_create_transposed_device", "tcsc_gpu_sgemm_t", "tcsc_gpu_prelu_backward",
    "tcsc_gpu_sgemm_bf16", "tcsc_gpu_launch_info_bf16",
    "tcsc_gpu_plan_enable_i8", "tcsc_gpu_plan_has_i8", "tcsc_gpu_sgemm_i8", "tcsc_gpu_launch_info_i8",
    "tcsc_gpu_quantize_rows_i8", "tcsc_gpu_workspace_bound_i8",
    "tcsc_gpu_plan_enable_w2", "tcsc_gpu_plan_has_w2", "tcsc_gpu_w2_image_bytes", "tcsc_gpu_decode_pays",
    "tcsc_gpu_launch_geometry", "tcsc_gpu_wide_pays", "tcsc_gpu_plan_wide_stats",
    "tcsc_gpu_plan_create_packed", "tcsc_gpu_plan_create_packed_device", "tcsc_gpu_plan_is_packed",
    "tcsc_gpu_plan_copy_w2",
    "tcsc_gpu_plan_create_packed_image", "tcsc_gpu_plan_create_packed_image_device", "tcsc_gpu_w2_to_tcsc",
    "tcsc_gpu_w2_from_tcsc_host", "tcsc_gpu_w2_to_tcsc_host",
    "tcsc_gpu_quantize_rows_i8_bf16", "tcsc_gpu_sgemm_q8", "tcsc_gpu_launch_info_q8", "tcsc_gpu_quant_fuse_pays",
    "tcsc_gpu_sgemm_i8_out", "tcsc_gpu_sgemm_q8_out",
    "tcsc_gpu_rmsnorm_rows", "tcsc_gpu_quantize_rows_i8_norm", "tcsc_gpu_sgemm_q8_norm",
    "tcsc_gpu_launch_info_q8_norm", "tcsc_gpu_norm_fuse_pays",
    "tcsc_gpu_sgemm_i8_glu", "tcsc_gpu_sgemm_q8_glu", "tcsc_gpu_launch_info_glu", "tcsc_gpu_glu_fuse_pays",
    "tcsc_gpu_sgemm_i8_group", "tcsc_gpu_sgemm_q8_group", "tcsc_gpu_launch_info_group", "tcsc_gpu_group_fuse_pays",
    "tcsc_gpu_sgemm_i8_res", "tcsc_gpu_sgemm_q8_res",
    "tcsc_gpu_plan_set_decode_rows", "tcsc_gpu_plan_decode_rows", "tcsc_gpu_decode_rows_pays",
    "tcsc_gpu_launch_info_decode",
    "tcsc_gpu_plan_set_decode_rows_multi", "tcsc_gpu_plan_decode_rows_multi", "tcsc_gpu_glu_rows_pays",
    "tcsc_gpu_group_rows_pays", "tcsc_gpu_launch_info_glu_decode", "tcsc_gpu_launch_info_group_decode",
    # include/sparse/bcsr.h
    "bcsr_from_dense", "bcsr_sgemm_basic", "bcsr_sgemm_prelu_basic", "bcsr_sgemm_avx", "bcsr_sgemm_prelu_avx",
    "bcsr_sgemm_avx2", "bcsr_free",
    # include/bcsr_gpu.h
    "bcsr_gpu_plan_create", "bcsr_gpu_plan_stats", "bcsr_gpu_plan_reserve", "bcsr_gpu_plan_destroy",
    "bcsr_gpu_sgemm", "bcsr_gpu_prepare_x", "bcsr_gpu_sgemm_prepared",
    # include/sparse_gemm.h (SparseGEMM.h's raw-array API)
    "tcsc_sparse_format", "tcsc_sparse_gemm", "tcsc_sparse_gemm_prelu", "tcsc_dense_gemm", "tcsc_dense_gemm_prelu",
)


class TcscError(RuntimeError):
    pass


class tcsc_t(C.Structure):
    """Layout of tcsc_t (include/sparse/tcsc.h; reference sparse/tcsc.h:6-17)."""

    _fields_ = [
        ("rows", C.c_int), ("cols", C.c_int), ("n_elem_pos", C.c_int), ("n_elem_neg", C.c_int),
        ("col_start_pos", C.POINTER(C.c_int)), ("col_start_neg", C.POINTER(C.c_int)),
        ("row_index_pos", C.POINTER(C.c_int)), ("row_index_neg", C.POINTER(C.c_int)),
    ]


class plan_info_t(C.Structure):
    _fields_ = [
        ("device", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("col_begin", C.c_int),
        ("nnz", C.c_longlong), ("n_pos", C.c_longlong), ("n_neg", C.c_longlong),
        ("chunk_k", C.c_int), ("n_chunks", C.c_int), ("device_bytes", C.c_size_t), ("order", C.c_int),
        ("mfma_min_M", C.c_int),
    ]


GROUP_MAX = 4  # TCSC_GROUP_MAX
DECODE_ROWS_AUTO = -1  # TCSC_DECODE_ROWS_AUTO


class group_member_t(C.Structure):
    """Layout of tcsc_gpu_group_member (include/tcsc_gpu.h): one matrix of a grouped int8 call."""

    _fields_ = [
        ("plan", C.c_void_p), ("dColScale", C.c_void_p), ("dB", C.c_void_p), ("dY", C.c_void_p), ("ldy", C.c_int),
    ]


_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_lib = None


def build(force: bool = False) -> str:
    """Compile lib/libtcsc_amd.so (hipcc --offload-arch=gfx950)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, "-j8"])
    return LIB_PATH


def lib():
    """Load the library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TcscError(f"{LIB_PATH} missing: build it with `make -C {PKG_DIR}`")
    # One HIP runtime per process: torch ships its own libamdhip64 (SONAME
    # libamdhip64.so.7, the one the library needs too).  Loaded first, it is
    # the one the library binds to; loaded after the library's
    # /opt/rocm copy, torch sees two runtimes and reports no device
    # (torch.cuda.is_available() False).  So bring torch in first when it is
    # installed; the library itself never calls into torch.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    # the timing-only diagnostic builds of tools/ab.mk compute wrong results by
    # design: never under a parity test or a bench line unless asked for
    L.tcsc_gpu_build_flags.restype = C.c_int
    flags = int(L.tcsc_gpu_build_flags())
    if flags and os.environ.get("TCSC_ALLOW_DIAG") != "1":
        raise TcscError(f"{LIB_PATH} is a diagnostic build (flags {flags:#x}: ablation/no-DMA/stamps/trace, "
                        "results wrong by design); set TCSC_ALLOW_DIAG=1 to load it anyway")
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    P = C.POINTER(tcsc_t)
    L.tcsc_from_dense.argtypes = [_f32p, i, i]
    L.tcsc_from_dense.restype = P
    for n in ("tcsc_sgemm_basic", "tcsc_sgemm_optimized"):
        getattr(L, n).argtypes = [_f32p, P, _f32p, _f32p, i, i, i]
        getattr(L, n).restype = None
    for n in ("tcsc_sgemm_prelu_basic", "tcsc_sgemm_prelu_optimized_separate",
              "tcsc_sgemm_prelu_optimized_onthego"):
        getattr(L, n).argtypes = [_f32p, P, _f32p, f, _f32p, i, i, i]
        getattr(L, n).restype = None
    L.tcsc_free.argtypes = [P]
    L.tcsc_free.restype = None
    L.tcsc_set_seed.argtypes = [C.c_ulonglong]
    L.tcsc_gpu_device_count.restype = i
    L.tcsc_gpu_last_error.restype = C.c_char_p
    L.tcsc_gpu_plan_create.argtypes = [P, i, i, i, vp, C.POINTER(vp)]
    L.tcsc_gpu_plan_create_device.argtypes = [i, i, vp, vp, vp, vp, i, i, i, vp, C.POINTER(vp)]
    L.tcsc_gpu_plan_get_info.argtypes = [vp, C.POINTER(plan_info_t)]
    L.tcsc_gpu_launch_info.argtypes = [vp, i, C.POINTER(i), C.POINTER(i)]
    L.tcsc_gpu_launch_combine.argtypes = [vp, i, C.POINTER(i)]
    L.tcsc_gpu_launch_geometry.argtypes = [vp, i, C.POINTER(i)]
    L.tcsc_gpu_wide_pays.argtypes = [i, i, i]
    L.tcsc_gpu_plan_wide_stats.argtypes = [vp, C.POINTER(C.c_longlong), vp, C.c_size_t]
    L.tcsc_gpu_plan_reserve.argtypes = [vp, i]
    L.tcsc_gpu_plan_workspace.argtypes = [vp, i, i, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.tcsc_gpu_plan_destroy.argtypes = [vp]
    L.tcsc_gpu_plan_destroy.restype = None
    L.tcsc_gpu_sgemm.argtypes = [vp, vp, vp, vp, i, i, i, f, vp]
    L.tcsc_gpu_sgemm_bf16.argtypes = [vp, vp, vp, vp, i, i, i, f, vp]
    L.tcsc_gpu_launch_info_bf16.argtypes = [vp, i, C.POINTER(i), C.POINTER(i)]
    L.tcsc_gpu_plan_enable_i8.argtypes = [vp, vp]
    L.tcsc_gpu_plan_has_i8.argtypes = [vp]
    L.tcsc_gpu_sgemm_i8.argtypes = [vp, vp, vp, vp, vp, i, i, i, f, vp]
    L.tcsc_gpu_launch_info_i8.argtypes = [vp, i, C.POINTER(i), C.POINTER(i)]
    L.tcsc_gpu_quantize_rows_i8.argtypes = [vp, i, i, vp, vp, vp]
    L.tcsc_gpu_workspace_bound_i8.argtypes = [i, i, i, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.tcsc_gpu_plan_enable_w2.argtypes = [vp, vp]
    L.tcsc_gpu_plan_has_w2.argtypes = [vp]
    L.tcsc_gpu_w2_image_bytes.argtypes = [i, i, C.POINTER(C.c_size_t)]
    L.tcsc_gpu_decode_pays.argtypes = [i, i, i, C.c_longlong]
    L.tcsc_gpu_plan_create_packed.argtypes = [P, i, i, i, vp, C.POINTER(vp)]
    L.tcsc_gpu_plan_create_packed_device.argtypes = [i, i, vp, vp, vp, vp, i, i, i, vp, C.POINTER(vp)]
    L.tcsc_gpu_plan_is_packed.argtypes = [vp]
    L.tcsc_gpu_plan_copy_w2.argtypes = [vp, vp, C.c_size_t, vp]
    L.tcsc_gpu_plan_create_packed_image.argtypes = [vp, C.c_size_t, i, i, i, i, vp, C.POINTER(vp)]
    L.tcsc_gpu_plan_create_packed_image_device.argtypes = [vp, C.c_size_t, i, i, i, i, vp, C.POINTER(vp)]
    L.tcsc_gpu_w2_to_tcsc.argtypes = [vp, C.c_size_t, i, i, vp, vp, vp, vp, C.POINTER(i), C.POINTER(i), vp]
    L.tcsc_gpu_w2_from_tcsc_host.argtypes = [P, i, i, vp, C.c_size_t]
    L.tcsc_gpu_w2_to_tcsc_host.argtypes = [vp, C.c_size_t, i, i]
    L.tcsc_gpu_w2_to_tcsc_host.restype = P
    L.tcsc_gpu_quantize_rows_i8_bf16.argtypes = [vp, i, i, vp, vp, vp]
    L.tcsc_gpu_sgemm_q8.argtypes = [vp, vp, i, vp, vp, vp, vp, i, i, i, f, vp]
    L.tcsc_gpu_launch_info_q8.argtypes = [vp, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.tcsc_gpu_quant_fuse_pays.argtypes = [i, i, i, i]
    L.tcsc_gpu_sgemm_i8_out.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, f, vp]
    L.tcsc_gpu_sgemm_q8_out.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, f, vp]
    L.tcsc_gpu_rmsnorm_rows.argtypes = [vp, i, vp, f, i, i, vp, vp, vp]
    L.tcsc_gpu_quantize_rows_i8_norm.argtypes = [vp, i, vp, f, i, i, vp, vp, vp]
    L.tcsc_gpu_sgemm_q8_norm.argtypes = [vp, vp, i, vp, f, vp, vp, vp, vp, vp, i, i, i, i, f, vp]
    L.tcsc_gpu_launch_info_q8_norm.argtypes = [vp, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.tcsc_gpu_norm_fuse_pays.argtypes = [i, i, i, i]
    L.tcsc_gpu_sgemm_i8_glu.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
    L.tcsc_gpu_sgemm_q8_glu.argtypes = [vp, vp, vp, i, vp, f, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
    L.tcsc_gpu_launch_info_glu.argtypes = [vp, vp, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.tcsc_gpu_glu_fuse_pays.argtypes = [i, i, i, i, i]
    gm = C.POINTER(group_member_t)
    L.tcsc_gpu_sgemm_i8_group.argtypes = [gm, i, vp, vp, i, i, vp]
    L.tcsc_gpu_sgemm_q8_group.argtypes = [gm, i, vp, i, vp, f, vp, vp, i, i, vp]
    L.tcsc_gpu_launch_info_group.argtypes = [gm, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.tcsc_gpu_group_fuse_pays.argtypes = [i, i, C.POINTER(i), i, i, i]
    L.tcsc_gpu_sgemm_i8_res.argtypes = [vp, vp, vp, vp, vp, vp, i, vp, i, i, i, vp]
    L.tcsc_gpu_sgemm_q8_res.argtypes = [vp, vp, i, vp, f, vp, vp, vp, vp, vp, i, vp, i, i, i, vp]
    L.tcsc_gpu_plan_set_decode_rows.argtypes = [vp, i]
    L.tcsc_gpu_plan_decode_rows.argtypes = [vp]
    L.tcsc_gpu_decode_rows_pays.argtypes = [i, i, i, i]
    L.tcsc_gpu_launch_info_decode.argtypes = [vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_longlong)]
    L.tcsc_gpu_plan_set_decode_rows_multi.argtypes = [vp, i]
    L.tcsc_gpu_plan_decode_rows_multi.argtypes = [vp]
    L.tcsc_gpu_glu_rows_pays.argtypes = [i, i, i, i]
    L.tcsc_gpu_group_rows_pays.argtypes = [i, i, C.POINTER(i), i, i]
    L.tcsc_gpu_launch_info_glu_decode.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_longlong)]
    L.tcsc_gpu_launch_info_group_decode.argtypes = [gm, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_longlong)]
    L.tcsc_gpu_prepare_x.argtypes = [vp, vp, i, vp]
    L.tcsc_gpu_sgemm_prepared.argtypes = [vp, vp, vp, i, i, i, f, vp]
    L.tcsc_gpu_from_dense.argtypes = [vp, i, i, vp, vp, vp, vp, C.POINTER(i), C.POINTER(i), vp]
    L.tcsc_gpu_dense_sgemm.argtypes = [vp, vp, vp, vp, i, i, i, i, i, f, vp]
    L.tcsc_gpu_transpose_index.argtypes = [i, i, vp, vp, vp, vp, i, i, vp, vp, vp, vp, vp]
    L.tcsc_gpu_plan_create_transposed.argtypes = [P, i, i, i, vp, C.POINTER(vp)]
    L.tcsc_gpu_plan_create_transposed_device.argtypes = [i, i, vp, vp, vp, vp, i, i, i, vp, C.POINTER(vp)]
    L.tcsc_gpu_sgemm_t.argtypes = [vp, vp, vp, i, i, vp]
    L.tcsc_gpu_prelu_backward.argtypes = [vp, i, vp, i, f, vp, i, vp, i, i, vp]
    L.tcsc_gpu_num_shards.restype = i
    L.tcsc_gpu_set_num_shards.argtypes = [i]
    L.tcsc_gpu_set_num_shards.restype = None
    L.tcsc_gpu_cache_clear.restype = None
    L.tcsc_gpu_set_order.argtypes = [i]
    L.tcsc_gpu_set_order.restype = None
    L.tcsc_gpu_get_order.restype = i
    ip = C.POINTER(i)
    L.tcsc_sparse_format.argtypes = [_i32p, i, i, _i32p, _i32p, vp, vp, ip, ip]
    L.tcsc_sparse_format.restype = i
    L.tcsc_sparse_gemm.argtypes = [_f32p, _i32p, _i32p, _i32p, _i32p, _f32p, _f32p, i, i, i]
    L.tcsc_sparse_gemm.restype = None
    L.tcsc_sparse_gemm_prelu.argtypes = L.tcsc_sparse_gemm.argtypes + [f]
    L.tcsc_sparse_gemm_prelu.restype = None
    L.tcsc_dense_gemm.argtypes = [_f32p, _f32p, _f32p, _f32p, i, i, i]
    L.tcsc_dense_gemm.restype = None
    L.tcsc_dense_gemm_prelu.argtypes = L.tcsc_dense_gemm.argtypes + [f]
    L.tcsc_dense_gemm_prelu.restype = None
    from . import bcsr as _bcsr

    _bcsr.bind(L)
    _lib = L
    return L


def last_error() -> str:
    return lib().tcsc_gpu_last_error().decode(errors="replace")


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise TcscError(f"{what} failed (status {rc}): {last_error()}")


def device_count() -> int:
    return int(lib().tcsc_gpu_device_count())


def require_gpu() -> None:
    if device_count() <= 0:
        raise TcscError("no HIP device visible: the TCSC kernels need a gfx950 (MI355X) GPU")


class TcscMatrix:
    """Owns a ``tcsc_t*`` (tcsc_from_dense / tcsc_free, sparse/tcsc.h:19,48)."""

    def __init__(self, ptr):
        if not ptr:
            raise TcscError("tcsc_from_dense returned NULL")
        self.ptr = ptr

    @classmethod
    def from_dense(cls, dense: np.ndarray) -> "TcscMatrix":
        dense = np.ascontiguousarray(dense, dtype=np.float32)
        rows, cols = dense.shape
        buf = dense.reshape(-1) if dense.size else np.zeros(1, np.float32)
        return cls(lib().tcsc_from_dense(buf, rows, cols))

    @classmethod
    def from_arrays(cls, rows: int, cols: int, col_start_pos, col_start_neg, row_index_pos,
                    row_index_neg) -> "TcscMatrix":
        """A hand-built ``tcsc_t`` (the struct of sparse/tcsc.h:6-17) from four
        index arrays, in malloc'd memory so that ``tcsc_free`` releases it as
        it releases ``tcsc_from_dense``'s.  No checks here: the library's
        plan build validates (rows in [0, rows), order) as the tests need."""
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        libc.malloc.argtypes = [C.c_size_t]

        def put(a):
            a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
            p = libc.malloc(max(a.nbytes, 4))
            if not p:
                raise MemoryError("malloc failed")
            if a.size:
                C.memmove(p, a.ctypes.data, a.nbytes)
            return C.cast(p, C.POINTER(C.c_int)), a.size

        t = libc.malloc(C.sizeof(tcsc_t))
        if not t:
            raise MemoryError("malloc failed")
        s = C.cast(t, C.POINTER(tcsc_t))
        s.contents.rows, s.contents.cols = int(rows), int(cols)
        s.contents.col_start_pos, _ = put(col_start_pos)
        s.contents.col_start_neg, _ = put(col_start_neg)
        s.contents.row_index_pos, s.contents.n_elem_pos = put(row_index_pos)
        s.contents.row_index_neg, s.contents.n_elem_neg = put(row_index_neg)
        return cls(s)

    def row_index(self, sign: str) -> np.ndarray:
        """Writable view of row_index_pos ('pos') or row_index_neg ('neg'):
        lets tests rebuild the arrays in place, as a caller may."""
        t = self.ptr.contents
        p, n = (t.row_index_pos, t.n_elem_pos) if sign == "pos" else (t.row_index_neg, t.n_elem_neg)
        return np.ctypeslib.as_array(p, shape=(n,)) if n > 0 else np.zeros(0, np.int32)

    @property
    def rows(self) -> int:
        return self.ptr.contents.rows

    @property
    def cols(self) -> int:
        return self.ptr.contents.cols

    @property
    def nnz(self) -> int:
        t = self.ptr.contents
        return t.n_elem_pos + t.n_elem_neg

    def arrays(self):
        """(col_start_pos, col_start_neg, row_index_pos, row_index_neg) copies."""
        t = self.ptr.contents

        def take(p, n):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n > 0 else np.zeros(0, np.int32)

        return (take(t.col_start_pos, t.cols + 1), take(t.col_start_neg, t.cols + 1),
                take(t.row_index_pos, t.n_elem_pos), take(t.row_index_neg, t.n_elem_neg))

    def free(self) -> None:
        if self.ptr:
            lib().tcsc_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sgemm(variant: str, X: np.ndarray, W: TcscMatrix, B: np.ndarray, a: float = 0.2,
          Y: np.ndarray | None = None) -> np.ndarray:
    """Host-pointer call of tcsc_sgemm_<variant> (sparse/tcsc.h:21-46).

    The C entry points trust their sizes as the reference's do (they read N
    floats of B and write M rows of pitch N into Y), so the shapes are checked
    here and a mismatch raises :class:`TcscError` instead of reaching the
    library as an out-of-bounds host read or write."""
    if variant not in VARIANTS:
        raise TcscError(f"unknown variant {variant!r} (one of {', '.join(VARIANTS)})")
    if not getattr(W, "ptr", None):
        raise TcscError("W is freed or not a TcscMatrix")
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise TcscError(f"X must be 2-D (M x K), got shape {X.shape}")
    M, K = X.shape
    N = W.cols
    if K != W.rows:
        raise TcscError(f"X has K={K} columns but W has {W.rows} rows")
    B = np.ascontiguousarray(B, dtype=np.float32).reshape(-1)
    if B.size != N:
        raise TcscError(f"B has {B.size} elements, W has N={N} columns")
    if Y is None:
        Y = np.empty((M, N), np.float32)
    elif (not isinstance(Y, np.ndarray) or Y.shape != (M, N) or Y.dtype != np.float32
          or not Y.flags["C_CONTIGUOUS"]):
        raise TcscError(f"Y must be a C-contiguous float32 array of shape ({M}, {N})")
    L = lib()
    nz = lambda a_: a_.reshape(-1) if a_.size else np.zeros(1, np.float32)  # noqa: E731
    if variant in PRELU_VARIANTS:
        name = "tcsc_sgemm_prelu_basic" if variant == "prelu_basic" else "tcsc_sgemm_" + variant.replace(
            "prelu_", "prelu_optimized_")
        getattr(L, name)(nz(X), W.ptr, nz(B), a, nz(Y), M, N, K)
    else:
        getattr(L, "tcsc_sgemm_" + variant)(nz(X), W.ptr, nz(B), nz(Y), M, N, K)
    return Y


# --- SparseGEMM.h's raw-array API (include/sparse_gemm.h) -------------------

def sparse_format(matrix: np.ndarray):
    """SparseFormat(int* matrix, K, N) (SparseGEMM.h:20-39): an int K x N
    matrix -> (col_start_pos, col_start_neg, row_index_pos, row_index_neg);
    >= 1 is +1, <= -1 is -1.  Host code in the library (no GPU needed)."""
    m = np.ascontiguousarray(matrix, dtype=np.int32)
    if m.ndim != 2:
        raise TcscError(f"matrix must be 2-D (K x N), got shape {m.shape}")
    K, N = m.shape
    flat = m.reshape(-1) if m.size else np.zeros(1, np.int32)
    csp, csn = np.zeros(N + 1, np.int32), np.zeros(N + 1, np.int32)
    p, q = C.c_int(0), C.c_int(0)
    L = lib()
    _check(L.tcsc_sparse_format(flat, K, N, csp, csn, None, None, C.byref(p), C.byref(q)), "tcsc_sparse_format")
    rip, rin = np.zeros(max(p.value, 1), np.int32), np.zeros(max(q.value, 1), np.int32)
    _check(L.tcsc_sparse_format(flat, K, N, csp, csn, rip.ctypes.data, rin.ctypes.data, C.byref(p), C.byref(q)),
           "tcsc_sparse_format")
    return csp, csn, rip[:p.value].copy(), rin[:q.value].copy()


def sparse_gemm(X: np.ndarray, col_start_pos, col_start_neg, row_index_pos, row_index_neg, b: np.ndarray,
                a: float | None = None, Y: np.ndarray | None = None) -> np.ndarray:
    """sparseGEMM<float> (a None) or sparseGEMM_PReLU<float> (SparseGEMM.h:104-119,
    151-168) on host arrays: Y = act(X . W + b), W given by its four TCSC
    arrays.  Shapes are checked here (the C entry points trust them)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise TcscError(f"X must be 2-D (M x K), got shape {X.shape}")
    M, K = X.shape
    arrs = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1)
            for v in (col_start_pos, col_start_neg, row_index_pos, row_index_neg)]
    csp, csn, rip, rin = arrs
    N = csp.size - 1
    if N < 0 or csn.size != N + 1:
        raise TcscError("col_start_pos / col_start_neg must both have N+1 entries")
    if rip.size < csp[-1] or rin.size < csn[-1]:
        raise TcscError("row_index arrays shorter than col_start[N]")
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    if b.size != N:
        raise TcscError(f"b has {b.size} elements, W has N={N} columns")
    if Y is None:
        Y = np.empty((M, N), np.float32)
    elif Y.shape != (M, N) or Y.dtype != np.float32 or not Y.flags["C_CONTIGUOUS"]:
        raise TcscError(f"Y must be a C-contiguous float32 array of shape ({M}, {N})")
    nz = lambda v, t: v if v.size else np.zeros(1, t)  # noqa: E731
    args = [nz(X.reshape(-1), np.float32), csp, csn, nz(rip, np.int32), nz(rin, np.int32), nz(b, np.float32),
            nz(Y.reshape(-1), np.float32), M, N, K]
    if a is None:
        lib().tcsc_sparse_gemm(*args)
    else:
        lib().tcsc_sparse_gemm_prelu(*args, float(a))
    return Y


def dense_gemm(X: np.ndarray, W: np.ndarray, b: np.ndarray, a: float | None = None) -> np.ndarray:
    """GEMM<float> / GEMM_PReLU<float> (SparseGEMM.h:121-149) on host arrays,
    computed by the GPU's fp32 rocBLAS product + bias/PReLU epilogue."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    if X.ndim != 2 or W.ndim != 2 or X.shape[1] != W.shape[0]:
        raise TcscError(f"X {X.shape} and W {W.shape} do not chain")
    M, K = X.shape
    N = W.shape[1]
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    if b.size != N:
        raise TcscError(f"b has {b.size} elements, W has N={N} columns")
    Y = np.empty((M, N), np.float32)
    nz = lambda v: v.reshape(-1) if v.size else np.zeros(1, np.float32)  # noqa: E731
    if a is None:
        lib().tcsc_dense_gemm(nz(X), nz(W), nz(b), nz(Y), M, N, K)
    else:
        lib().tcsc_dense_gemm_prelu(nz(X), nz(W), nz(b), nz(Y), M, N, K, float(a))
    return Y


ORDERS = {"fast": 0, "reference": 1}


def set_order(order: str) -> None:
    """Summation order of plans created from now on (include/tcsc_gpu.h
    tcsc_order): "fast" (merged +1/-1, tolerance parity) or "reference"
    (each variant's own order: float outputs bit-identical to the reference)."""
    lib().tcsc_gpu_set_order(ORDERS[order])


def get_order() -> str:
    return {v: k for k, v in ORDERS.items()}[int(lib().tcsc_gpu_get_order())]


def set_num_shards(n: int) -> None:
    lib().tcsc_gpu_set_num_shards(int(n))


def num_shards() -> int:
    return int(lib().tcsc_gpu_num_shards())


def cache_clear() -> None:
    lib().tcsc_gpu_cache_clear()


def _ptr(x) -> int:
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):  # torch tensor
        return int(x.data_ptr())
    raise TypeError(f"expected a device pointer or tensor, got {type(x)}")


class Plan:
    """Device plan for columns [col_begin, col_end) of W (include/tcsc_gpu.h)."""

    def __init__(self, W: TcscMatrix, col_begin: int = 0, col_end: int | None = None, device: int = 0,
                 stream: int = 0):
        col_end = W.cols if col_end is None else col_end
        h = C.c_void_p()
        _check(lib().tcsc_gpu_plan_create(W.ptr, col_begin, col_end, device, C.c_void_p(stream), C.byref(h)),
               "tcsc_gpu_plan_create")
        self.handle = h

    @classmethod
    def from_device(cls, rows, cols, csp, csn, rip, rin, col_begin=0, col_end=None, device=0, stream=0):
        self = cls.__new__(cls)
        col_end = cols if col_end is None else col_end
        h = C.c_void_p()
        _check(lib().tcsc_gpu_plan_create_device(rows, cols, C.c_void_p(_ptr(csp)), C.c_void_p(_ptr(csn)),
                                                 C.c_void_p(_ptr(rip)), C.c_void_p(_ptr(rin)), col_begin,
                                                 col_end, device, C.c_void_p(stream), C.byref(h)),
               "tcsc_gpu_plan_create_device")
        self.handle = h
        return self

    @classmethod
    def transposed(cls, W: TcscMatrix, col_begin: int = 0, col_end: int | None = None, device: int = 0,
                   stream: int = 0) -> "Plan":
        """The plan of W[:, col_begin:col_end]^T (tcsc_gpu_plan_create_transposed): an ordinary
        plan of col_end - col_begin rows and W.rows columns, for :meth:`sgemm_t`."""
        if not getattr(W, "ptr", None):
            raise TcscError("W is freed or not a TcscMatrix")
        self = cls.__new__(cls)
        col_end = W.cols if col_end is None else col_end
        h = C.c_void_p()
        _check(lib().tcsc_gpu_plan_create_transposed(W.ptr, col_begin, col_end, device, C.c_void_p(stream),
                                                     C.byref(h)), "tcsc_gpu_plan_create_transposed")
        self.handle = h
        return self

    @classmethod
    def transposed_from_device(cls, rows, cols, csp, csn, rip, rin, col_begin=0, col_end=None, device=0,
                               stream=0) -> "Plan":
        """Same from W's TCSC arrays on the device (tcsc_gpu_plan_create_transposed_device)."""
        self = cls.__new__(cls)
        col_end = cols if col_end is None else col_end
        h = C.c_void_p()
        _check(lib().tcsc_gpu_plan_create_transposed_device(rows, cols, C.c_void_p(_ptr(csp)), C.c_void_p(_ptr(csn)),
                                                            C.c_void_p(_ptr(rip)), C.c_void_p(_ptr(rin)), col_begin,
                                                            col_end, device, C.c_void_p(stream), C.byref(h)),
               "tcsc_gpu_plan_create_transposed_device")
        self.handle = h
        return self

    @classmethod
    def packed(cls, W: TcscMatrix, col_begin: int = 0, col_end: int | None = None, device: int = 0,
               stream: int = 0) -> "Plan":
        """A packed plan of W[:, col_begin:col_end] (tcsc_gpu_plan_create_packed): the 2-bit image and nothing
        else of W, a quarter byte per weight.  Only :meth:`sgemm_i8` runs on it -- k_decode8 up to 16 rows,
        k_gemm8w2 above -- with the bits of an ordinary plan's int8 MFMA path; every other call raises.
        TcscError when W is not ternary (a duplicated index), K >= 2^22, or the reference order is set."""
        if not getattr(W, "ptr", None):
            raise TcscError("W is freed or not a TcscMatrix")
        self = cls.__new__(cls)
        col_end = W.cols if col_end is None else col_end
        h = C.c_void_p()
        _check(lib().tcsc_gpu_plan_create_packed(W.ptr, col_begin, col_end, device, C.c_void_p(stream), C.byref(h)),
               "tcsc_gpu_plan_create_packed")
        self.handle = h
        return self

    @classmethod
    def packed_from_device(cls, rows, cols, csp, csn, rip, rin, col_begin=0, col_end=None, device=0,
                           stream=0) -> "Plan":
        """Same from W's TCSC arrays on the device (tcsc_gpu_plan_create_packed_device)."""
        self = cls.__new__(cls)
        col_end = cols if col_end is None else col_end
        h = C.c_void_p()
        _check(lib().tcsc_gpu_plan_create_packed_device(rows, cols, C.c_void_p(_ptr(csp)), C.c_void_p(_ptr(csn)),
                                                        C.c_void_p(_ptr(rip)), C.c_void_p(_ptr(rin)), col_begin,
                                                        col_end, device, C.c_void_p(stream), C.byref(h)),
               "tcsc_gpu_plan_create_packed_device")
        self.handle = h
        return self

    @classmethod
    def packed_from_image(cls, image, rows: int, cols: int, col_begin: int = 0, device: int = 0,
                          stream: int = 0) -> "Plan":
        """A packed plan from a saved 2-bit image of a rows x cols W: a numpy uint8 array (host memory,
        tcsc_gpu_plan_create_packed_image) or a contiguous device tensor / device pointer of
        w2_image_bytes(rows, cols) bytes (tcsc_gpu_plan_create_packed_image_device).  The plan owns a copy.
        col_begin only labels info()['col_begin'] (a column shard's image).  TcscError when the size is wrong,
        K >= 2^22, the reference order is set, or the image holds a code 3 or non-canonical padding."""
        self = cls.__new__(cls)
        h = C.c_void_p()
        if isinstance(image, np.ndarray):
            if image.dtype != np.uint8:
                raise TcscError(f"Plan.packed_from_image: a host image must be uint8, got {image.dtype}")
            host = np.ascontiguousarray(image).reshape(-1)
            ptr, nbytes, name = host.ctypes.data, host.size, "tcsc_gpu_plan_create_packed_image"
        else:
            if hasattr(image, "is_contiguous") and not image.is_contiguous():
                raise TcscError("Plan.packed_from_image: the device image must be contiguous")
            nbytes = image.numel() * image.element_size() if hasattr(image, "numel") else w2_image_bytes(rows, cols)
            ptr, name = _ptr(image), "tcsc_gpu_plan_create_packed_image_device"
        _check(getattr(lib(), name)(C.c_void_p(ptr), int(nbytes), int(rows), int(cols), int(col_begin), int(device),
                                    C.c_void_p(stream), C.byref(h)), name)
        self.handle = h
        return self

    @property
    def is_packed(self) -> bool:
        return bool(lib().tcsc_gpu_plan_is_packed(self.handle))

    def w2_image(self, stream: int = 0):
        """A new torch.uint8 device tensor holding the plan's 2-bit image (:meth:`copy_w2` into it, asynchronous
        on the stream): what :meth:`packed_from_image` and :func:`w2_to_tcsc` take."""
        import torch

        inf = self.info()
        img = torch.empty(w2_image_bytes(inf["rows"], inf["cols"]), dtype=torch.uint8,
                          device=torch.device("cuda", inf["device"]))
        self.copy_w2(img, stream=stream)
        return img

    def copy_w2(self, dst, nbytes: int | None = None, stream: int = 0) -> None:
        """Copy the plan's 2-bit image (device to device, asynchronous on the stream) into dst: a contiguous
        device tensor, whose size is passed as it is, or a pointer with nbytes (tcsc_gpu_plan_copy_w2).
        TcscError on a plan without the image, or when the size is not w2_image_bytes(K, cols)."""
        if nbytes is None:
            nbytes = dst.numel() * dst.element_size() if hasattr(dst, "numel") else 0
        _check(lib().tcsc_gpu_plan_copy_w2(self.handle, C.c_void_p(_ptr(dst)), int(nbytes), C.c_void_p(stream)),
               "tcsc_gpu_plan_copy_w2")

    def info(self) -> dict:
        inf = plan_info_t()
        _check(lib().tcsc_gpu_plan_get_info(self.handle, C.byref(inf)), "tcsc_gpu_plan_get_info")
        return {k: getattr(inf, k) for k, _ in plan_info_t._fields_}

    def _launch_info(self, name: str, M: int) -> tuple[str, int]:
        path, slices = C.c_int(), C.c_int()
        _check(getattr(lib(), name)(self.handle, int(M), C.byref(path), C.byref(slices)), name)
        return ("gather", "fused", "mfma", "small", "decode")[path.value], slices.value

    def launch_info(self, M: int) -> tuple[str, int]:
        """(path, K slices) of a launch of M rows: path is 'gather' (k_transpose +
        k_stream), 'mfma' or 'small' (include/tcsc_gpu.h tcsc_gpu_launch_info; value 1,
        the retired persistent k_fused, is never returned)."""
        return self._launch_info("tcsc_gpu_launch_info", M)

    def launch_info_bf16(self, M: int) -> tuple[str, int]:
        """(path, K slices) of an :meth:`sgemm_bf16` launch of M rows (tcsc_gpu_launch_info_bf16): the bf16
        call has its own cost model (a one-part GEMM), so its path can differ from :meth:`launch_info`'s."""
        return self._launch_info("tcsc_gpu_launch_info_bf16", M)

    def launch_combine(self, M: int) -> bool:
        """True when a gather launch of M rows combines its split-K slabs inside
        k_stream instead of a k_reduce launch (tcsc_gpu_launch_combine)."""
        return self.combine_mode(M) is not None

    def combine_mode(self, M: int):
        """How a gather launch of M rows combines its split-K slabs: 'pairwise'
        (2 slices, inside k_stream, any grid), 'pairwise-split' (2 slices, split
        halves, a resident grid), 'bands' (>= 3 slices, inside k_stream) or None
        (k_reduce4 after it, or no split) -- tcsc_gpu_launch_combine."""
        v = C.c_int()
        _check(lib().tcsc_gpu_launch_combine(self.handle, int(M), C.byref(v)), "tcsc_gpu_launch_combine")
        return {2: "bands", 3: "pairwise", 4: "pairwise-split"}.get(v.value)

    def launch_geometry(self, M: int) -> int:
        """Columns per wave of a gather launch of M rows: 16 (k_stream), 22 (k_stream_w, the wide
        geometry) or 0 when the launch is not on the gather path (tcsc_gpu_launch_geometry)."""
        v = C.c_int()
        _check(lib().tcsc_gpu_launch_geometry(self.handle, int(M), C.byref(v)), "tcsc_gpu_launch_geometry")
        return v.value

    def wide_stats(self) -> dict:
        """The slot map of the plan's 22-column streams and its statistics (tcsc_gpu_plan_wide_stats):
        ``map`` is a (column blocks, 16 waves, 22 slots) uint16 array of block-local columns;
        ``max_identity`` / ``max_balanced`` are the sums over blocks and chunks of the busiest wave's
        entries under contiguous columns and under the map in use; ``long_identity`` / ``long_balanced``
        count the (wave, chunk) streams longer than the kernel's 30-entry scalar buffer.  TcscError on a
        plan whose reserve built no wide streams."""
        st = (C.c_longlong * 4)()
        nblk = (self.info()["cols"] + 351) // 352
        m = np.empty((nblk, 16, 22), np.uint16)
        _check(lib().tcsc_gpu_plan_wide_stats(self.handle, st, C.c_void_p(m.ctypes.data), m.size),
               "tcsc_gpu_plan_wide_stats")
        return dict(max_identity=st[0], max_balanced=st[1], long_identity=st[2], long_balanced=st[3], map=m)

    def reserve(self, max_M: int) -> None:
        """Allocate the workspace (X^T + split-K slabs) for launches of up to max_M rows."""
        _check(lib().tcsc_gpu_plan_reserve(self.handle, int(max_M)), "tcsc_gpu_plan_reserve")

    PATH_ID = {None: -1, "gather": 0, "mfma": 2, "small": 3, "decode": 4}

    def workspace(self, M: int, path: str | None = None) -> tuple[int, int]:
        """(bytes a launch of M rows wants, bytes reserved now): host arithmetic, no
        launch.  path None: the path launch_info(M) names; 'gather', 'mfma' or
        'small': that path's need at M whatever the cost model prefers, 0 where the
        plan cannot run it; 'decode': always 0, the decode path reads X in place
        (tcsc_gpu_plan_workspace)."""
        need, reserved = C.c_size_t(), C.c_size_t()
        _check(lib().tcsc_gpu_plan_workspace(self.handle, int(M), self.PATH_ID[path], C.byref(need),
                                             C.byref(reserved)), "tcsc_gpu_plan_workspace")
        return need.value, reserved.value

    def sgemm(self, X, B, Y, M: int, ldy: int, variant: str = "prelu_basic", a: float = 0.2,
              stream: int = 0) -> None:
        _check(lib().tcsc_gpu_sgemm(self.handle, C.c_void_p(_ptr(X)), C.c_void_p(_ptr(B)), C.c_void_p(_ptr(Y)),
                                    int(M), int(ldy), VARIANT_ID[variant], float(a), C.c_void_p(stream)),
               "tcsc_gpu_sgemm")

    def sgemm_bf16(self, X, B, Y, M: int, ldy: int, variant: str = "prelu_basic", a: float = 0.2,
                   stream: int = 0) -> None:
        """:meth:`sgemm` for bf16 activations (tcsc_gpu_sgemm_bf16): X is M x K contiguous bf16 (a
        torch.bfloat16 tensor, or a pointer to uint16 bit patterns); B and Y stay fp32.  The bits are
        those of sgemm on X widened to fp32 on the same path and K split."""
        _check(lib().tcsc_gpu_sgemm_bf16(self.handle, C.c_void_p(_ptr(X)), C.c_void_p(_ptr(B)), C.c_void_p(_ptr(Y)),
                                         int(M), int(ldy), VARIANT_ID[variant], float(a), C.c_void_p(stream)),
               "tcsc_gpu_sgemm_bf16")

    def enable_i8(self, stream: int = 0) -> bool:
        """Build the int8 image of W beside the bf16 MFMA image (tcsc_gpu_plan_enable_i8) and return
        :attr:`has_i8`: False on a gather-only or reference-order plan, or when a weight does not fit int8 --
        :meth:`sgemm_i8` then runs the gather or the small-M path.  Idempotent; synchronises the stream."""
        _check(lib().tcsc_gpu_plan_enable_i8(self.handle, C.c_void_p(stream)), "tcsc_gpu_plan_enable_i8")
        return self.has_i8

    @property
    def has_i8(self) -> bool:
        return bool(lib().tcsc_gpu_plan_has_i8(self.handle))

    def launch_info_i8(self, M: int) -> tuple[str, int]:
        """(path, K slices) of an :meth:`sgemm_i8` launch of M rows (tcsc_gpu_launch_info_i8); the path may be
        'decode' (k_decode8 on the 2-bit image: M <= 16 after :meth:`enable_w2`)."""
        return self._launch_info("tcsc_gpu_launch_info_i8", M)

    def enable_w2(self, stream: int = 0) -> bool:
        """Build the 2-bit image of a ternary W beside the int8 image (tcsc_gpu_plan_enable_w2) and return
        :attr:`has_w2`: False on a plan without the int8 image, when a weight is not -1, 0 or +1 (a duplicated
        index) or K >= 2^22 -- :meth:`sgemm_i8` then runs as before.  With the image, int8 calls of M <= 16 rows
        may take the decode path (:func:`decode_pays`, $TCSC_DECODE).  Idempotent; synchronises the stream."""
        _check(lib().tcsc_gpu_plan_enable_w2(self.handle, C.c_void_p(stream)), "tcsc_gpu_plan_enable_w2")
        return self.has_w2

    @property
    def has_w2(self) -> bool:
        return bool(lib().tcsc_gpu_plan_has_w2(self.handle))

    def set_decode_rows(self, rows: int) -> None:
        """The most rows an int8 call on this plan takes to the decode path (tcsc_gpu_plan_set_decode_rows):
        16 .. 64 -- above 16 the row-tiled k_decode8r, one launch and no workspace -- or
        :data:`DECODE_ROWS_AUTO` for wherever :func:`decode_rows_pays` says so.  The default, 16, routes every
        call as before.  Needs the 2-bit image; allocates nothing and does not synchronise."""
        _check(lib().tcsc_gpu_plan_set_decode_rows(self.handle, int(rows)), "tcsc_gpu_plan_set_decode_rows")

    @property
    def decode_rows(self) -> int:
        """The setting of :meth:`set_decode_rows` (tcsc_gpu_plan_decode_rows)."""
        return int(lib().tcsc_gpu_plan_decode_rows(self.handle))

    def set_decode_rows_multi(self, rows: int) -> None:
        """The most rows a gated or grouped int8 call takes to the decode path where every plan of the call says
        so (tcsc_gpu_plan_set_decode_rows_multi): 16 .. 64, or :data:`DECODE_ROWS_AUTO` for wherever
        :func:`glu_rows_pays` / :func:`group_rows_pays` say so.  The default, 16, routes every call as before;
        :meth:`set_decode_rows` is not read by those calls.  Needs the 2-bit image; allocates nothing."""
        _check(lib().tcsc_gpu_plan_set_decode_rows_multi(self.handle, int(rows)), "tcsc_gpu_plan_set_decode_rows_multi")

    @property
    def decode_rows_multi(self) -> int:
        """The setting of :meth:`set_decode_rows_multi` (tcsc_gpu_plan_decode_rows_multi)."""
        return int(lib().tcsc_gpu_plan_decode_rows_multi(self.handle))

    def launch_info_decode(self, M: int) -> tuple[int, int, int]:
        """(row tiles, column tiles per workgroup, workgroups) of a decode launch of M rows on this plan
        (tcsc_gpu_launch_info_decode), whether or not M routes there: 1 <= M <= 64 on a plan with the image."""
        rt, ct, wg = C.c_int(0), C.c_int(0), C.c_longlong(0)
        _check(lib().tcsc_gpu_launch_info_decode(self.handle, int(M), C.byref(rt), C.byref(ct), C.byref(wg)),
               "tcsc_gpu_launch_info_decode")
        return rt.value, ct.value, wg.value

    def sgemm_i8(self, Xq, scale, B, Y, M: int, ldy: int, variant: str = "prelu_basic", a: float = 0.2,
                 stream: int = 0, col_scale=None, ytype=None, residual=None, ldr=None) -> None:
        """Y = act(scale[m] * col_scale[j] * (Xq . W) + B) for int8 activations (tcsc_gpu_sgemm_i8_out): Xq is
        M x K contiguous int8 (a torch.int8 tensor or a pointer), scale M floats or None for all ones, col_scale
        the plan's cols floats or None for all ones; B is fp32.  Y is fp32 or bf16, ldy in its elements: a
        tensor's dtype says which, a raw pointer is fp32 unless ytype ('f32' / 'bf16') says otherwise.  A
        col_scale or a bf16 Y needs the decode or the MFMA route (:meth:`launch_info_i8`): TcscError elsewhere.

        residual (tcsc_gpu_sgemm_i8_res): M x ldr elements of Y's type (ldr defaults to ldy), added to the value
        in the epilogue as one fp32 add ahead of the one rounding to Y's type; it may be Y itself with ldr ==
        ldy (in place).  The variant must then be 'basic', and the route decode or MFMA."""
        yt = _ytype_of(Y) if ytype is None else _ytype(ytype)
        if residual is not None:
            _res_check(residual, yt, variant)
            _check(lib().tcsc_gpu_sgemm_i8_res(self.handle, C.c_void_p(_ptr(Xq)), C.c_void_p(_ptr(scale)),
                                               C.c_void_p(_ptr(col_scale)), C.c_void_p(_ptr(B)),
                                               C.c_void_p(_ptr(residual)), int(ldy if ldr is None else ldr),
                                               C.c_void_p(_ptr(Y)), yt, int(M), int(ldy), C.c_void_p(stream)),
                   "tcsc_gpu_sgemm_i8_res")
            return
        _check(lib().tcsc_gpu_sgemm_i8_out(self.handle, C.c_void_p(_ptr(Xq)), C.c_void_p(_ptr(scale)),
                                           C.c_void_p(_ptr(col_scale)), C.c_void_p(_ptr(B)), C.c_void_p(_ptr(Y)), yt,
                                           int(M), int(ldy), VARIANT_ID[variant], float(a), C.c_void_p(stream)),
               "tcsc_gpu_sgemm_i8_out")

    def sgemm_q8(self, X, Xq, scale, B, Y, M: int, ldy: int, variant: str = "prelu_basic", a: float = 0.2,
                 stream: int = 0, xtype=None, col_scale=None, ytype=None, residual=None, ldr=None) -> None:
        """The quantizer and :meth:`sgemm_i8` in one call (tcsc_gpu_sgemm_q8_out): X is M x K contiguous fp32 or
        bf16 (a torch tensor, whose dtype says which, or a pointer with xtype 'f32' / 'bf16'), scale (M floats) is
        written, Xq (M x K int8) is scratch -- untouched, and allowed to be None, where the call is fused
        (:meth:`launch_info_q8`).  Y and scale get the bits of :func:`quantize_rows_i8` + :meth:`sgemm_i8`;
        col_scale, the type of Y, ytype, residual and ldr as there (tcsc_gpu_sgemm_q8_res)."""
        xt = _xtype_of(X) if xtype is None else _xtype(xtype)
        yt = _ytype_of(Y) if ytype is None else _ytype(ytype)
        if residual is not None:
            _res_check(residual, yt, variant)
            self._sgemm_q8_res(X, xt, None, 0.0, Xq, scale, col_scale, B, residual, ldy if ldr is None else ldr, Y, yt,
                               M, ldy, stream)
            return
        _check(lib().tcsc_gpu_sgemm_q8_out(self.handle, C.c_void_p(_ptr(X)), xt, C.c_void_p(_ptr(Xq)),
                                           C.c_void_p(_ptr(scale)), C.c_void_p(_ptr(col_scale)), C.c_void_p(_ptr(B)),
                                           C.c_void_p(_ptr(Y)), yt, int(M), int(ldy), VARIANT_ID[variant], float(a),
                                           C.c_void_p(stream)), "tcsc_gpu_sgemm_q8_out")

    def launch_info_q8(self, M: int, dtype="f32") -> tuple[str, int, bool]:
        """(path, K slices, fused) of an :meth:`sgemm_q8` launch of M rows of that dtype ('f32', 'bf16' or a
        torch dtype): the int8 route, and whether the quantizer runs inside the decode kernel
        (tcsc_gpu_launch_info_q8)."""
        path, slices, fused = C.c_int(), C.c_int(), C.c_int()
        _check(lib().tcsc_gpu_launch_info_q8(self.handle, int(M), _xtype(dtype), C.byref(path), C.byref(slices),
                                             C.byref(fused)), "tcsc_gpu_launch_info_q8")
        return ("gather", "fused", "mfma", "small", "decode")[path.value], slices.value, bool(fused.value)

    def sgemm_q8_norm(self, X, Xq, scale, B, Y, M: int, ldy: int, norm_weight=None, eps: float = 1e-6,
                      variant: str = "prelu_basic", a: float = 0.2, stream: int = 0, xtype=None, col_scale=None,
                      ytype=None, residual=None, ldr=None) -> None:
        """:meth:`sgemm_q8` on RMSNorm(X) * norm_weight (tcsc_gpu_sgemm_q8_norm): norm_weight is K floats or None
        for all ones.  Y and scale get the bits of :func:`rmsnorm_rows` + :func:`quantize_rows_i8` +
        :meth:`sgemm_i8`; one launch where the call is fused (:meth:`launch_info_q8_norm`: Xq is then untouched and
        may be None), :func:`quantize_rows_i8_norm` into Xq and the int8 call elsewhere.  residual and ldr as in
        :meth:`sgemm_i8` (tcsc_gpu_sgemm_q8_res with the norm; eps must not be 0 there)."""
        xt = _xtype_of(X) if xtype is None else _xtype(xtype)
        yt = _ytype_of(Y) if ytype is None else _ytype(ytype)
        if residual is not None:
            _res_check(residual, yt, variant)
            if float(eps) == 0.0:
                raise TcscError("sgemm_q8_norm: eps == 0 means no norm on the residual call; use sgemm_q8")
            self._sgemm_q8_res(X, xt, norm_weight, eps, Xq, scale, col_scale, B, residual, ldy if ldr is None else ldr,
                               Y, yt, M, ldy, stream)
            return
        _check(lib().tcsc_gpu_sgemm_q8_norm(self.handle, C.c_void_p(_ptr(X)), xt, C.c_void_p(_ptr(norm_weight)),
                                            float(eps), C.c_void_p(_ptr(Xq)), C.c_void_p(_ptr(scale)),
                                            C.c_void_p(_ptr(col_scale)), C.c_void_p(_ptr(B)), C.c_void_p(_ptr(Y)), yt,
                                            int(M), int(ldy), VARIANT_ID[variant], float(a), C.c_void_p(stream)),
               "tcsc_gpu_sgemm_q8_norm")

    def _sgemm_q8_res(self, X, xt, norm_weight, eps, Xq, scale, col_scale, B, residual, ldr, Y, yt, M, ldy,
                      stream) -> None:
        _check(lib().tcsc_gpu_sgemm_q8_res(self.handle, C.c_void_p(_ptr(X)), xt, C.c_void_p(_ptr(norm_weight)),
                                           float(eps), C.c_void_p(_ptr(Xq)), C.c_void_p(_ptr(scale)),
                                           C.c_void_p(_ptr(col_scale)), C.c_void_p(_ptr(B)),
                                           C.c_void_p(_ptr(residual)), int(ldr), C.c_void_p(_ptr(Y)), yt, int(M),
                                           int(ldy), C.c_void_p(stream)), "tcsc_gpu_sgemm_q8_res")

    def launch_info_q8_norm(self, M: int, dtype="f32") -> tuple[str, int, bool]:
        """(path, K slices, fused) of an :meth:`sgemm_q8_norm` launch of M rows of that dtype
        (tcsc_gpu_launch_info_q8_norm): the int8 route, and whether norm, quantizer and GEMM are one kernel."""
        path, slices, fused = C.c_int(), C.c_int(), C.c_int()
        _check(lib().tcsc_gpu_launch_info_q8_norm(self.handle, int(M), _xtype(dtype), C.byref(path), C.byref(slices),
                                                  C.byref(fused)), "tcsc_gpu_launch_info_q8_norm")
        return ("gather", "fused", "mfma", "small", "decode")[path.value], slices.value, bool(fused.value)

    def sgemm_t(self, G, DX, M: int, ldx: int, stream: int = 0) -> None:
        """dX (M x K, pitch ldx) = G (M x plan rows, contiguous) . W[:, range]^T on a transposed
        plan (tcsc_gpu_sgemm_t); TcscError on a plan that :meth:`transposed` did not make."""
        _check(lib().tcsc_gpu_sgemm_t(self.handle, C.c_void_p(_ptr(G)), C.c_void_p(_ptr(DX)), int(M), int(ldx),
                                      C.c_void_p(stream)), "tcsc_gpu_sgemm_t")

    def prepare_x(self, X, M: int, stream: int = 0) -> None:
        """First half of sgemm: stage X^T in the plan's workspace (k_transpose)."""
        _check(lib().tcsc_gpu_prepare_x(self.handle, C.c_void_p(_ptr(X)), int(M), C.c_void_p(stream)),
               "tcsc_gpu_prepare_x")

    def sgemm_prepared(self, B, Y, M: int, ldy: int, variant: str = "prelu_basic", a: float = 0.2,
                       stream: int = 0) -> None:
        """Second half of sgemm: the gather on the staged X^T (k_stream)."""
        _check(lib().tcsc_gpu_sgemm_prepared(self.handle, C.c_void_p(_ptr(B)), C.c_void_p(_ptr(Y)), int(M), int(ldy),
                                             VARIANT_ID[variant], float(a), C.c_void_p(stream)),
               "tcsc_gpu_sgemm_prepared")

    def destroy(self) -> None:
        if getattr(self, "handle", None):
            lib().tcsc_gpu_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def dense_sgemm(X, Wd, B, Y, M: int, N: int, K: int, ldy: int, variant: str = "prelu_basic", a: float = 0.2,
                stream: int = 0) -> None:
    """Dense baseline on the device (gemm_basic, dense/dense.c:64-77): Y = act(X Wd + B), rocBLAS fp32 SGEMM
    plus the bias/PReLU epilogue kernel.  X, Wd, B, Y are device buffers (torch tensors or raw pointers)."""
    _check(lib().tcsc_gpu_dense_sgemm(C.c_void_p(_ptr(X)), C.c_void_p(_ptr(Wd)), C.c_void_p(_ptr(B)),
                                      C.c_void_p(_ptr(Y)), int(M), int(N), int(K), int(ldy), VARIANT_ID[variant],
                                      float(a), C.c_void_p(stream)), "tcsc_gpu_dense_sgemm")


def gpu_from_dense(d_dense, rows: int, cols: int, d_csp, d_csn, d_rip=None, d_rin=None, stream: int = 0):
    """Device tcsc_from_dense; returns (n_pos, n_neg)."""
    p, q = C.c_int(), C.c_int()
    _check(lib().tcsc_gpu_from_dense(C.c_void_p(_ptr(d_dense)), rows, cols, C.c_void_p(_ptr(d_csp)),
                                     C.c_void_p(_ptr(d_csn)), C.c_void_p(_ptr(d_rip)), C.c_void_p(_ptr(d_rin)),
                                     C.byref(p), C.byref(q), C.c_void_p(stream)), "tcsc_gpu_from_dense")
    return p.value, q.value


def gpu_transpose_index(rows: int, cols: int, d_csp, d_csn, d_rip, d_rin, col_begin: int, col_end: int, d_t_csp,
                        d_t_csn, d_t_rip, d_t_rin, stream: int = 0) -> None:
    """Device transpose of the index structure (tcsc_gpu_transpose_index): the TCSC arrays of W (rows x cols) ->
    those of W[:, col_begin:col_end]^T; d_t_csp / d_t_csn hold rows + 1 ints, d_t_rip / d_t_rin the range's
    n_pos / n_neg ints.  Synchronises the stream."""
    _check(lib().tcsc_gpu_transpose_index(int(rows), int(cols), C.c_void_p(_ptr(d_csp)), C.c_void_p(_ptr(d_csn)),
                                          C.c_void_p(_ptr(d_rip)), C.c_void_p(_ptr(d_rin)), int(col_begin),
                                          int(col_end), C.c_void_p(_ptr(d_t_csp)), C.c_void_p(_ptr(d_t_csn)),
                                          C.c_void_p(_ptr(d_t_rip)), C.c_void_p(_ptr(d_t_rin)), C.c_void_p(stream)),
           "tcsc_gpu_transpose_index")


XTYPE_ID = {"f32": 0, "bf16": 1}


def _xtype(spec) -> int:
    """enum tcsc_xtype of 'f32' / 'bf16', a torch dtype, or the enum's own integer (passed on as it is)."""
    if isinstance(spec, int):
        return spec
    if isinstance(spec, str) and spec in XTYPE_ID:
        return XTYPE_ID[spec]
    name = str(spec)
    if name in ("torch.float32", "torch.bfloat16"):
        return int(name == "torch.bfloat16")
    raise TcscError(f"activations must be fp32 or bf16 ('f32', 'bf16' or the torch dtype), got {spec!r}")


def _xtype_of(X) -> int:
    """enum tcsc_xtype of a buffer: a tensor's dtype says; a raw pointer or None counts as fp32."""
    dt = getattr(X, "dtype", None)
    return 0 if dt is None else _xtype(dt)


YTYPE_ID = {"f32": 0, "bf16": 1}


def _ytype(spec) -> int:
    """enum tcsc_ytype of 'f32' / 'bf16', a torch dtype, or the enum's own integer (passed on as it is)."""
    if isinstance(spec, int):
        return spec
    if isinstance(spec, str) and spec in YTYPE_ID:
        return YTYPE_ID[spec]
    name = str(spec)
    if name in ("torch.float32", "torch.bfloat16"):
        return int(name == "torch.bfloat16")
    raise TcscError(f"Y must be fp32 or bf16 ('f32', 'bf16' or the torch dtype), got {spec!r}")


def _ytype_of(Y) -> int:
    """enum tcsc_ytype of an output buffer: a tensor's dtype says; a raw pointer or None counts as fp32."""
    dt = getattr(Y, "dtype", None)
    return 0 if dt is None else _ytype(dt)


def _res_check(residual, yt: int, variant: str) -> None:
    """What a residual asks of a Plan.sgemm_i8 / sgemm_q8 / sgemm_q8_norm call: no PReLU, and Y's dtype."""
    if variant != "basic":
        raise TcscError(f"a residual goes with variant 'basic' alone (no PReLU), not {variant!r}")
    if hasattr(residual, "dtype") and _ytype_of(residual) != yt:
        raise TcscError(f"the residual's dtype {residual.dtype} is not Y's")


def ternarize_absmean(Wf):
    """The absmean rule of ternary-weight models, on the host (numpy only, no device): for a float matrix Wf,
    beta = mean |W| in fp32 and T = clip(rint(W / beta), -1, 1) as int8, so that W ~ beta * T.  rint rounds ties
    to even: |w| = 0.5 beta gives 0, |w| = 1.5 beta gives +-1 by the clip.  An all-zero (or empty) W gives
    beta 0 and T zeros.  Returns (T, beta) with beta a numpy float32; T is what :class:`TcscMatrix.from_dense`
    and ``PackedTernaryLinear`` take, beta the layer's per-tensor ``weight_scale``."""
    W = np.ascontiguousarray(Wf, dtype=np.float32)
    beta = np.float32(np.mean(np.abs(W), dtype=np.float32)) if W.size else np.float32(0.0)
    if not beta > 0:
        return np.zeros(W.shape, dtype=np.int8), np.float32(0.0)
    return np.clip(np.rint(W / beta), -1, 1).astype(np.int8), beta


def quantize_rows_i8(X, Xq, scale, M: int, K: int, stream: int = 0) -> None:
    """Per-row absmax quantization on the device (tcsc_gpu_quantize_rows_i8, or _bf16 for a torch.bfloat16 X):
    X is M x K contiguous fp32 or bf16; Xq (M x K int8) and scale (M floats) are written: scale = amax / 127,
    q = clamp(rint(x * (127 / amax)), -127, 127), a row of zeros gives q = 0 and scale = 0, and so does a row whose
    maximum is so small that 127 / amax is inf in fp32 (amax <= 127 * 2^-128, about 3.73e-37, and every subnormal
    maximum): zero = not (amax > 0) or isinf(127 / amax).  bf16 values are widened to fp32 first (exact)."""
    name = "tcsc_gpu_quantize_rows_i8_bf16" if _xtype_of(X) else "tcsc_gpu_quantize_rows_i8"
    _check(getattr(lib(), name)(C.c_void_p(_ptr(X)), int(M), int(K), C.c_void_p(_ptr(Xq)),
                                C.c_void_p(_ptr(scale)), C.c_void_p(stream)), name)


def quant_fuse_pays(M: int, K: int, N: int, dtype="f32") -> bool:
    """The default rule for fusing the quantizer into the decode call (tcsc_gpu_quant_fuse_pays; host
    arithmetic): whether :meth:`Plan.sgemm_q8` of M rows of that dtype on a K x N decode route runs one kernel."""
    return bool(lib().tcsc_gpu_quant_fuse_pays(int(M), int(K), int(N), _xtype(dtype)))


def rmsnorm_rows(X, Xn, M: int, K: int, weight=None, eps: float = 1e-6, rinv=None, stream: int = 0, xtype=None) -> None:
    """RMSNorm of the rows of X in the library's pinned arithmetic (tcsc_gpu_rmsnorm_rows): X is M x K contiguous
    fp32 or bf16, weight K floats or None for all ones; Xn (M x K floats) = fl(fl(x * r) * weight) with
    r = 1 / sqrt(mean(x^2) + eps), the sum of squares in a fixed order; rinv (M floats), where given, gets r."""
    xt = _xtype_of(X) if xtype is None else _xtype(xtype)
    _check(lib().tcsc_gpu_rmsnorm_rows(C.c_void_p(_ptr(X)), xt, C.c_void_p(_ptr(weight)), float(eps), int(M), int(K),
                                       C.c_void_p(_ptr(Xn)), C.c_void_p(_ptr(rinv)), C.c_void_p(stream)),
           "tcsc_gpu_rmsnorm_rows")


def quantize_rows_i8_norm(X, Xq, scale, M: int, K: int, weight=None, eps: float = 1e-6, stream: int = 0,
                          xtype=None) -> None:
    """:func:`rmsnorm_rows` and :func:`quantize_rows_i8` in one launch, the same bits
    (tcsc_gpu_quantize_rows_i8_norm): Xq (M x K int8) and scale (M floats) are written."""
    xt = _xtype_of(X) if xtype is None else _xtype(xtype)
    _check(lib().tcsc_gpu_quantize_rows_i8_norm(C.c_void_p(_ptr(X)), xt, C.c_void_p(_ptr(weight)), float(eps), int(M),
                                                int(K), C.c_void_p(_ptr(Xq)), C.c_void_p(_ptr(scale)),
                                                C.c_void_p(stream)), "tcsc_gpu_quantize_rows_i8_norm")


def norm_fuse_pays(M: int, K: int, N: int, dtype="f32") -> bool:
    """The default rule for fusing norm and quantizer into the decode call (tcsc_gpu_norm_fuse_pays; host
    arithmetic): whether :meth:`Plan.sgemm_q8_norm` of M rows of that dtype on a K x N decode route runs one
    kernel."""
    return bool(lib().tcsc_gpu_norm_fuse_pays(int(M), int(K), int(N), _xtype(dtype)))


GLU_ACT_ID = {"relu2": 0, "silu": 1}


def _glu_act(act) -> int:
    """enum tcsc_glu_act of 'relu2' / 'silu', or the enum's own integer (passed on as it is)."""
    if isinstance(act, int):
        return act
    if act in GLU_ACT_ID:
        return GLU_ACT_ID[act]
    raise TcscError(f"the gate activation must be one of {sorted(GLU_ACT_ID)}, got {act!r}")


def launch_info_glu(gate_plan, up_plan, M: int, dtype="f32") -> tuple[str, int, bool]:
    """(path, K slices, fused) of a gated call of M rows (tcsc_gpu_launch_info_glu): 'decode' up to 16 rows -- up
    to 64 where both plans' :meth:`Plan.set_decode_rows_multi` setting admits M -- and 'mfma' above; fused: whether :func:`sgemm_q8_glu` of that dtype, without a norm, quantizes inside the launch."""
    path, slices, fused = C.c_int(), C.c_int(), C.c_int()
    _check(lib().tcsc_gpu_launch_info_glu(gate_plan.handle, up_plan.handle, int(M), _xtype(dtype), C.byref(path),
                                          C.byref(slices), C.byref(fused)), "tcsc_gpu_launch_info_glu")
    return ("gather", "fused", "mfma", "small", "decode")[path.value], slices.value, bool(fused.value)


def _glu_scratch(gate_plan, up_plan, M: int, Y, G):
    """dG of a gated call: the caller's, or M x cols floats beside a tensor Y where the route is the MFMA one."""
    if G is not None or launch_info_glu(gate_plan, up_plan, M)[0] != "mfma" or not hasattr(Y, "new_empty"):
        return G
    import torch

    return Y.new_empty((int(M), gate_plan.info()["cols"]), dtype=torch.float32)


def sgemm_i8_glu(gate_plan, up_plan, Xq, scale, bias_gate, bias_up, Y, M: int, ldy: int, act="relu2",
                 col_scale_gate=None, col_scale_up=None, G=None, stream: int = 0, ytype=None) -> None:
    """Y = act(g) * u for int8 activations (tcsc_gpu_sgemm_i8_glu): g and u are :meth:`Plan.sgemm_i8` of Xq on the
    gate and the up plan (same K and cols, both with the 2-bit image) with their own column scales and biases
    and no PReLU; act is 'relu2' (relu(g)^2) or 'silu'.  Y is fp32 or bf16 by the tensor's dtype (a raw pointer:
    ytype).  G, the fp32 scratch for g (M x cols) on the MFMA route (M > 16), is allocated here when it is None
    and Y is a tensor; a captured call passes its own."""
    yt = _ytype_of(Y) if ytype is None else _ytype(ytype)
    G = _glu_scratch(gate_plan, up_plan, M, Y, G)
    _check(lib().tcsc_gpu_sgemm_i8_glu(gate_plan.handle, up_plan.handle, C.c_void_p(_ptr(Xq)), C.c_void_p(_ptr(scale)),
                                       C.c_void_p(_ptr(col_scale_gate)), C.c_void_p(_ptr(bias_gate)),
                                       C.c_void_p(_ptr(col_scale_up)), C.c_void_p(_ptr(bias_up)), C.c_void_p(_ptr(G)),
                                       C.c_void_p(_ptr(Y)), yt, int(M), int(ldy), _glu_act(act), C.c_void_p(stream)),
           "tcsc_gpu_sgemm_i8_glu")


def sgemm_q8_glu(gate_plan, up_plan, X, Xq, scale, bias_gate, bias_up, Y, M: int, ldy: int, act="relu2",
                 col_scale_gate=None, col_scale_up=None, norm_weight=None, norm_eps=None, G=None, stream: int = 0,
                 xtype=None, ytype=None) -> None:
    """The quantizer and :func:`sgemm_i8_glu` in one call (tcsc_gpu_sgemm_q8_glu): X is M x K fp32 or bf16, scale
    (M floats) is written and Xq (M x K int8) is scratch, untouched where the call is fused
    (:func:`launch_info_glu`).  norm_eps None: no norm (norm_weight must be None too); otherwise the RMSNorm of
    :meth:`Plan.sgemm_q8_norm` runs in front of the quantizer."""
    xt = _xtype_of(X) if xtype is None else _xtype(xtype)
    yt = _ytype_of(Y) if ytype is None else _ytype(ytype)
    G = _glu_scratch(gate_plan, up_plan, M, Y, G)
    _check(lib().tcsc_gpu_sgemm_q8_glu(gate_plan.handle, up_plan.handle, C.c_void_p(_ptr(X)), xt,
                                       C.c_void_p(_ptr(norm_weight)), 0.0 if norm_eps is None else float(norm_eps),
                                       C.c_void_p(_ptr(Xq)), C.c_void_p(_ptr(scale)), C.c_void_p(_ptr(col_scale_gate)),
                                       C.c_void_p(_ptr(bias_gate)), C.c_void_p(_ptr(col_scale_up)),
                                       C.c_void_p(_ptr(bias_up)), C.c_void_p(_ptr(G)), C.c_void_p(_ptr(Y)), yt, int(M),
                                       int(ldy), _glu_act(act), C.c_void_p(stream)), "tcsc_gpu_sgemm_q8_glu")


def launch_info_glu_decode(gate_plan, up_plan, M: int) -> tuple[int, int, int]:
    """(row tiles, column tiles per workgroup, workgroups) of a gated decode launch of M rows
    (tcsc_gpu_launch_info_glu_decode), whether or not M routes there: 1 <= M <= 64."""
    rt, ct, wg = C.c_int(), C.c_int(), C.c_longlong()
    _check(lib().tcsc_gpu_launch_info_glu_decode(gate_plan.handle, up_plan.handle, int(M), C.byref(rt), C.byref(ct),
                                                 C.byref(wg)), "tcsc_gpu_launch_info_glu_decode")
    return rt.value, ct.value, wg.value


def glu_rows_pays(M: int, K: int, H: int, num_cus: int = 0) -> bool:
    """Where the gated row-tiled decode launch of 16 < M <= 64 rows beats the MFMA route (tcsc_gpu_glu_rows_pays;
    host arithmetic): what plans set to :data:`DECODE_ROWS_AUTO` ask per gated call."""
    return bool(lib().tcsc_gpu_glu_rows_pays(int(M), int(K), int(H), int(num_cus)))


def glu_fuse_pays(M: int, K: int, N: int, dtype="f32", norm: bool = False) -> bool:
    """The default rule for fusing the quantizer (norm: and the norm) into the gated decode launch
    (tcsc_gpu_glu_fuse_pays; host arithmetic)."""
    return bool(lib().tcsc_gpu_glu_fuse_pays(int(M), int(K), int(N), _xtype(dtype), int(bool(norm))))


def _group_members(plans, biases=None, Ys=None, ldys=None, col_scales=None):
    """The tcsc_gpu_group_member array of a grouped call (and its length, passed on as it is: the library
    refuses a count outside 1 .. GROUP_MAX).  ldys None: every Y's own row pitch (a tensor's stride(0)), else
    the plan's column count."""
    n = len(plans)
    arr = (group_member_t * max(n, 1))()
    for k, plan in enumerate(plans):
        m = arr[k]
        m.plan = plan.handle if plan is not None else None
        m.dColScale = _ptr(col_scales[k]) if col_scales is not None and col_scales[k] is not None else None
        m.dB = _ptr(biases[k]) if biases is not None and biases[k] is not None else None
        Y = Ys[k] if Ys is not None else None
        m.dY = _ptr(Y) if Y is not None else None
        if ldys is not None:
            m.ldy = int(ldys[k])
        elif hasattr(Y, "stride") and hasattr(Y, "dim") and Y.dim() == 2:
            m.ldy = int(Y.stride(0))
        elif plan is not None and Ys is not None:
            m.ldy = plan.info()["cols"]
    return arr, n


def launch_info_group(plans, M: int, dtype="f32") -> tuple[str, list[int], bool]:
    """(path, [K slices of each member], fused) of a grouped call of M rows (tcsc_gpu_launch_info_group): 'decode'
    up to 16 rows -- up to 64 where every plan's :meth:`Plan.set_decode_rows_multi` setting admits M -- and 'mfma'
    above; fused: whether :func:`sgemm_q8_group` of that dtype, without a norm,
    quantizes inside the launch (with a norm it never does)."""
    arr, n = _group_members(plans)
    path, fused = C.c_int(), C.c_int()
    slices = (C.c_int * max(n, 1))()
    _check(lib().tcsc_gpu_launch_info_group(arr, n, int(M), _xtype(dtype), C.byref(path), slices, C.byref(fused)),
           "tcsc_gpu_launch_info_group")
    return ("gather", "fused", "mfma", "small", "decode")[path.value], [slices[k] for k in range(n)], bool(fused.value)


def _group_ytype(Ys, ytype) -> int:
    if ytype is not None:
        return _ytype(ytype)
    yts = {_ytype_of(Y) for Y in Ys}
    if not yts:  # an empty group: the library's refusal
        return 0
    if len(yts) != 1:
        raise TcscError("a grouped call writes one Y type: the outputs must share a dtype")
    return yts.pop()


def sgemm_i8_group(plans, Xq, scale, biases, Ys, M: int, ldys=None, col_scales=None, stream: int = 0,
                   ytype=None) -> None:
    """Several matrices on one int8 X in one call (tcsc_gpu_sgemm_i8_group): Ys[k] gets the bits of
    :meth:`Plan.sgemm_i8` of Xq on plans[k] (1 .. GROUP_MAX plans of one K, each with the 2-bit image) with
    biases[k], col_scales[k] (None: ones) and no PReLU.  The Ys are fp32 or bf16 alike, by the tensors' dtype
    (raw pointers: ytype), and may be column slices of one tensor; ldys None takes each tensor's row pitch.  Up
    to 16 rows it is one decode launch over all members, above one k_pack8 and one GEMM per member."""
    arr, n = _group_members(plans, biases, Ys, ldys, col_scales)
    _check(lib().tcsc_gpu_sgemm_i8_group(arr, n, C.c_void_p(_ptr(Xq)), C.c_void_p(_ptr(scale)), _group_ytype(Ys, ytype),
                                         int(M), C.c_void_p(stream)), "tcsc_gpu_sgemm_i8_group")


def sgemm_q8_group(plans, X, Xq, scale, biases, Ys, M: int, ldys=None, col_scales=None, norm_weight=None,
                   norm_eps=None, stream: int = 0, xtype=None, ytype=None) -> None:
    """The quantizer and :func:`sgemm_i8_group` in one call (tcsc_gpu_sgemm_q8_group): X is M x K fp32 or bf16,
    scale (M floats) is written and Xq (M x K int8) is scratch, untouched where the call is fused
    (:func:`launch_info_group`).  norm_eps None: no norm (norm_weight must be None too); otherwise the RMSNorm of
    :meth:`Plan.sgemm_q8_norm` runs in front of the quantizer, always in the quantizer's own launch."""
    xt = _xtype_of(X) if xtype is None else _xtype(xtype)
    arr, n = _group_members(plans, biases, Ys, ldys, col_scales)
    _check(lib().tcsc_gpu_sgemm_q8_group(arr, n, C.c_void_p(_ptr(X)), xt, C.c_void_p(_ptr(norm_weight)),
                                         0.0 if norm_eps is None else float(norm_eps), C.c_void_p(_ptr(Xq)),
                                         C.c_void_p(_ptr(scale)), _group_ytype(Ys, ytype), int(M), C.c_void_p(stream)),
           "tcsc_gpu_sgemm_q8_group")


def launch_info_group_decode(plans, M: int) -> tuple[int, int, int]:
    """(row tiles, column tiles per workgroup, workgroups) of a grouped decode launch of M rows
    (tcsc_gpu_launch_info_group_decode), whether or not M routes there: 1 <= M <= 64."""
    arr, n = _group_members(plans)
    rt, ct, wg = C.c_int(), C.c_int(), C.c_longlong()
    _check(lib().tcsc_gpu_launch_info_group_decode(arr, n, int(M), C.byref(rt), C.byref(ct), C.byref(wg)),
           "tcsc_gpu_launch_info_group_decode")
    return rt.value, ct.value, wg.value


def group_rows_pays(M: int, K: int, cols, num_cus: int = 0) -> bool:
    """Where the grouped row-tiled decode launch of 16 < M <= 64 rows over members with these column counts beats
    the MFMA route (tcsc_gpu_group_rows_pays; host arithmetic): what plans set to :data:`DECODE_ROWS_AUTO` ask
    per grouped call."""
    cols = [int(c) for c in cols]
    arr = (C.c_int * max(len(cols), 1))(*cols)
    return bool(lib().tcsc_gpu_group_rows_pays(int(M), int(K), arr, len(cols), int(num_cus)))


def group_fuse_pays(M: int, K: int, cols, dtype="f32", norm: bool = False) -> bool:
    """The default rule for fusing the quantizer into the grouped decode launch of members with these column
    counts (tcsc_gpu_group_fuse_pays; host arithmetic); False with the norm."""
    cols = [int(c) for c in cols]
    arr = (C.c_int * max(len(cols), 1))(*cols)
    return bool(lib().tcsc_gpu_group_fuse_pays(int(M), int(K), arr, len(cols), _xtype(dtype), int(bool(norm))))


def w2_image_bytes(K: int, N: int) -> int:
    """Bytes of the 2-bit image of a K x N ternary W: ceil(N/16) * ceil(K/256) * 1024 (tcsc_gpu_w2_image_bytes;
    host arithmetic, no device)."""
    b = C.c_size_t()
    _check(lib().tcsc_gpu_w2_image_bytes(int(K), int(N), C.byref(b)), "tcsc_gpu_w2_image_bytes")
    return b.value


def decode_pays(M: int, K: int, N: int, nnz: int) -> bool:
    """The default rule for the decode path (tcsc_gpu_decode_pays; host arithmetic): 1 <= M <= 16 and (M > 4, or
    the small-M path does not fit (M, K), or 16 * nnz > K * N)."""
    return bool(lib().tcsc_gpu_decode_pays(int(M), int(K), int(N), int(nnz)))


def decode_rows_pays(M: int, K: int, N: int, num_cus: int = 0) -> bool:
    """Where a row-tiled decode launch of 16 < M <= 64 rows beats the MFMA route (tcsc_gpu_decode_rows_pays; host
    arithmetic): what a plan set to :data:`DECODE_ROWS_AUTO` asks per call."""
    return bool(lib().tcsc_gpu_decode_rows_pays(int(M), int(K), int(N), int(num_cus)))


def w2_to_tcsc(image, rows: int, cols: int, stream: int = 0):
    """The TCSC arrays of the rows x cols matrix a 2-bit image on the device encodes (tcsc_gpu_w2_to_tcsc):
    (col_start_pos, col_start_neg, row_index_pos, row_index_neg) as torch.int32 tensors on the image's device, bit
    for bit tcsc_from_dense's of that matrix -- what :meth:`Plan.from_device` takes.  image is a contiguous device
    tensor of w2_image_bytes(rows, cols) bytes.  TcscError on an invalid image.  Synchronises the stream."""
    import torch

    if not torch.is_tensor(image) or not image.is_cuda or not image.is_contiguous():
        raise TcscError("w2_to_tcsc: image must be a contiguous CUDA tensor")
    nbytes = image.numel() * image.element_size()
    rows, cols = int(rows), int(cols)
    L, p, q = lib(), C.c_int(), C.c_int()
    with torch.cuda.device(image.device):
        csp = torch.empty(max(cols, 0) + 1, dtype=torch.int32, device=image.device)
        csn = torch.empty_like(csp)

        def call(rip, rin):
            _check(L.tcsc_gpu_w2_to_tcsc(C.c_void_p(_ptr(image)), nbytes, rows, cols, C.c_void_p(_ptr(csp)),
                                         C.c_void_p(_ptr(csn)), C.c_void_p(_ptr(rip)), C.c_void_p(_ptr(rin)),
                                         C.byref(p), C.byref(q), C.c_void_p(stream)), "tcsc_gpu_w2_to_tcsc")

        call(None, None)
        # at least one element each: an empty tensor's NULL pointer would ask for the counts again
        rip = torch.empty(max(p.value, 1), dtype=torch.int32, device=image.device)
        rin = torch.empty(max(q.value, 1), dtype=torch.int32, device=image.device)
        call(rip, rin)
    return csp, csn, rip[:p.value], rin[:q.value]


def w2_pack_host(W: TcscMatrix, col_begin: int = 0, col_end: int | None = None) -> np.ndarray:
    """The 2-bit image of W[:, col_begin:col_end] as a numpy uint8 array, made in host code
    (tcsc_gpu_w2_from_tcsc_host; no device needed): byte for byte the image of ``Plan.packed`` of the same range.
    TcscError when W is not ternary (a duplicated index), a row is outside [0, K) or K >= 2^22."""
    if not getattr(W, "ptr", None):
        raise TcscError("W is freed or not a TcscMatrix")
    col_end = W.cols if col_end is None else col_end
    nbytes = _w2_bytes(W.rows, col_end - col_begin)
    if nbytes is None:
        raise TcscError(f"w2_pack_host: no image for K={W.rows} and columns [{col_begin}, {col_end})")
    image = np.empty(nbytes, np.uint8)
    _check(lib().tcsc_gpu_w2_from_tcsc_host(W.ptr, int(col_begin), int(col_end), C.c_void_p(image.ctypes.data),
                                            nbytes), "tcsc_gpu_w2_from_tcsc_host")
    return image


def w2_unpack_host(image: np.ndarray, rows: int, cols: int) -> TcscMatrix:
    """The TcscMatrix a 2-bit image (numpy uint8) encodes, made in host code (tcsc_gpu_w2_to_tcsc_host; no device
    needed): the arrays tcsc_from_dense gives for that rows x cols matrix.  TcscError on an invalid image."""
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8:
        raise TcscError("w2_unpack_host: image must be a numpy uint8 array")
    host = np.ascontiguousarray(image).reshape(-1)
    ptr = lib().tcsc_gpu_w2_to_tcsc_host(C.c_void_p(host.ctypes.data), host.size, int(rows), int(cols))
    if not ptr:
        raise TcscError(f"tcsc_gpu_w2_to_tcsc_host failed: {last_error()}")
    return TcscMatrix(ptr)


PACKED_FORMAT_VERSION = 1


def _w2_bytes(rows: int, cols: int):
    """w2_image_bytes in Python (no library call), or None where no image exists (K < 1, K >= 2^22, no column)."""
    if not (1 <= rows < 1 << 22) or cols < 1:
        return None
    return ((cols + 15) // 16) * ((rows + 255) // 256) * 1024


def save_packed(plan: Plan, path) -> None:
    """Store one plan's 2-bit image as an .npz (np.savez, no pickle): `image` (uint8), `rows`, `cols`,
    `col_begin` and `version`.  Any plan that has the image can be saved; :func:`load_packed` gives a packed plan.
    path is a file name (np.savez appends .npz when it is missing) or a binary file object."""
    inf = plan.info()
    img = plan.w2_image()
    np.savez(path, image=img.cpu().numpy(), rows=np.int64(inf["rows"]), cols=np.int64(inf["cols"]),
             col_begin=np.int64(inf["col_begin"]), version=np.int64(PACKED_FORMAT_VERSION))


def load_packed(path, device: int = 0, stream: int = 0) -> Plan:
    """The packed plan of a file :func:`save_packed` wrote (np.load with allow_pickle=False).  The version, the
    image's dtype and its size for (rows, cols) are checked first: a file that fails raises TcscError before the
    library is called.  The file carries no runtime setting: :meth:`Plan.set_decode_rows` on the plan returned
    sets one."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("image", "rows", "cols", "col_begin", "version") if k not in z.files]
        if missing:
            raise TcscError(f"load_packed: {path}: missing {', '.join(missing)}")
        version, image = z["version"], z["image"]
        if version.shape != () or version.dtype.kind not in "iu" or int(version) != PACKED_FORMAT_VERSION:
            raise TcscError(f"load_packed: {path}: format version {version!r}, this library reads "
                            f"{PACKED_FORMAT_VERSION}")
        dims = [z[k] for k in ("rows", "cols", "col_begin")]
    if any(d.shape != () or d.dtype.kind not in "iu" for d in dims):
        raise TcscError(f"load_packed: {path}: rows, cols and col_begin must be integer scalars")
    rows, cols, col_begin = (int(d) for d in dims)
    if image.dtype != np.uint8:
        raise TcscError(f"load_packed: {path}: image has dtype {image.dtype}, expected uint8")
    want = _w2_bytes(rows, cols)
    if want is None or col_begin < 0 or image.size != want:
        raise TcscError(f"load_packed: {path}: image has {image.size} bytes, rows={rows} cols={cols} "
                        f"col_begin={col_begin} need {want}")
    return Plan.packed_from_image(image, rows, cols, col_begin, device, stream)


def prelu_backward(G, Y, a: float, DZ, DB, M: int, N: int, ldg: int | None = None, ldy: int | None = None,
                   lddz: int | None = None, stream: int = 0) -> None:
    """dZ = where(Y < 0, a * G, G) and db = dZ.sum(0) on the device (tcsc_gpu_prelu_backward).  Y None: the
    identity activation; DZ may be G (in place) or None; DB may be None.  Pitches default to N."""
    N = int(N)
    _check(lib().tcsc_gpu_prelu_backward(C.c_void_p(_ptr(G)), N if ldg is None else int(ldg), C.c_void_p(_ptr(Y)),
                                         N if ldy is None else int(ldy), float(a), C.c_void_p(_ptr(DZ)),
                                         N if lddz is None else int(lddz), C.c_void_p(_ptr(DB)), int(M), N,
                                         C.c_void_p(stream)), "tcsc_gpu_prelu_backward")
