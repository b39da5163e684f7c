// tcsc_api.cpp -- the device-pointer half of the C ABI of libtcsc_amd.so:
// include/tcsc_gpu.h (plans, the cost models and the route of a call,
// workspace, async launches, the backward pass).  The host-pointer half
// (include/sparse/tcsc.h, include/sparse_gemm.h) is tcsc_host.cpp, which
// reaches this file only through tcsc_plan.h; struct tcsc_gpu_plan is private
// to this file.
//
// Errors are recorded per thread (tcsc_gpu_last_error()) and returned as a
// status; what the void host API does with one is tcsc_host.cpp's policy.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sparse/tcsc.h"
#include "../../include/tcsc_gpu.h"
#include "tcsc_plan.h"

struct tcsc_gpu_plan {
    int device = 0;
    int rows = 0, cols = 0, col_begin = 0;
    long long n_pos = 0, n_neg = 0;
    int n_chunks = 0, n_groups = 0;
    long long n_entries = 0;
    int2* ent = nullptr;   // stream entries (+ guard batch)
    int* sptr = nullptr;   // stream starts, n_chunks*n_groups + 1
    float* ws = nullptr;   // X^T + split-K partial slabs (tcsc_gpu_plan_reserve)
    size_t ws_bytes = 0;
    size_t bytes = 0;
    // M of the X that tcsc_gpu_prepare_x left in ws (X^T's pitch depends on
    // it), or -1 when nothing is staged: never staged, the workspace was
    // reallocated, or a whole tcsc_gpu_sgemm overwrote it with its own X
    int staged_M = -1;
    // TCSC_ORDER_REFERENCE plans also carry the +1-only and -1-only chains
    // (plans of the column range with one sign each), which the kernel walks
    // one after the other in the reference's summation order
    int order = TCSC_ORDER_FAST;
    tcsc_gpu_plan* chain_pos = nullptr;
    tcsc_gpu_plan* chain_neg = nullptr;
    // MFMA path for denser W (tcsc_mfma.hip): W^T in bf16,
    // stored once (cols x mfma_ldw(rows)); the rows the bf16 split of X
    // cannot carry are recomputed from the CSC copy below.  Launches with
    // M >= mfma_min_M may take it (use_mfma); null when the plan is gather-only.
    uint16_t* wt = nullptr;
    size_t mfma_bytes = 0;
    // the int8 image of W^T beside it (cols x mfma8_ldw(rows) bytes), built
    // only by tcsc_gpu_plan_enable_i8: tcsc_gpu_sgemm_i8's MFMA path
    int8_t* w8 = nullptr;
    size_t i8_bytes = 0;
    // the 2-bit image of a ternary W made from it (w2_image_bytes(rows, cols)),
    // built only by tcsc_gpu_plan_enable_w2: int8 calls of M <= 16 rows stream
    // it (k_decode8)
    uint32_t* w2 = nullptr;
    size_t w2_bytes = 0;
    // the most rows an int8 call takes to the decode path (tcsc_gpu_plan_set_decode_rows):
    // 16 .. 64, above 16 the row-tiled k_decode8r, or TCSC_DECODE_ROWS_AUTO: wherever
    // tcsc_gpu_decode_rows_pays says so.  A setting only: it owns no memory
    int decode_rows = tcsc::kDecodeMaxM;
    // the same for the gated and grouped calls (tcsc_gpu_plan_set_decode_rows_multi): a call of
    // 16 < M <= 64 rows decodes (k_decode8gr / k_decode8mr) where every plan of the call admits M
    int decode_rows_multi = tcsc::kDecodeMaxM;
    // the column range's rebased CSC (fast-order plans): the small-M path
    // walks it, the MFMA path's fixup recomputes flagged rows from it
    // (crq: each column's +1 / -1 rows merged in ascending k, in the quad
    // layout of 64-column groups whose quad offsets are ccq: tcsc_internal.h)
    int *ccq = nullptr, *crq = nullptr;
    size_t csc_bytes = 0;
    int mfma_min_M = 0;
    // the in-launch split-K combine's tile words (tcsc::kCombineBytes, zeroed
    // when allocated; every completed launch leaves them at zero) and the CU
    // count its residency rule needs.  A launch that fails to enqueue marks
    // them dirty and the next launch re-zeroes them first.
    unsigned* csync = nullptr;
    mutable bool csync_dirty = false;
    int num_cus = 0;
    // the second copy of the entry streams, re-grouped for the 22-column
    // geometry (k_stream_w, DESIGN.md §4 "Two geometries"): built from ent /
    // sptr by tcsc_gpu_plan_reserve (or the reserve a launch falls into) where
    // wide_pays holds for a reserved M or $TCSC_GEO=22 asks for it; fast-order
    // plans only
    int2* ent_w = nullptr;
    int* sptr_w = nullptr;
    long long n_entries_w = 0;
    int n_groups_w = 0;
    // the wide streams' slot map (which columns of a column block each wave
    // owns: tcsc::wide_blocks_for(cols) x 352 entries, k_wide_balance) and its
    // statistics as tcsc_gpu_plan_wide_stats reports them
    unsigned short* wperm = nullptr;
    long long wide_stats[4] = {0, 0, 0, 0};
    size_t wide_bytes = 0;
    // transposed plans (tcsc_gpu_plan_create_transposed*): `cols` zeros, the
    // bias tcsc_gpu_sgemm_t hands to the launch; null on every other plan
    float* tbias = nullptr;
    size_t tbias_bytes = 0;
    // packed plans (tcsc_gpu_plan_create_packed*): w2 above is
    // all the plan holds of W -- no entry streams, no CSC copy, no bf16 or int8
    // image, no chains, no combine words -- and only int8 calls run on it:
    // k_decode8 at M <= 16, k_pack8 + k_gemm8w2 above
    bool packed = false;
};

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace tcsc {

void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int hip_fail(hipError_t e, const char* what) {
    set_error("%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    return TCSC_E_HIP;
}

void set_error_msg(const char* msg) { g_last_error = msg ? msg : ""; }
const char* error_msg() { return g_last_error.c_str(); }

int device_count_raw() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

}  // namespace tcsc

namespace {

using tcsc::current_order;
using tcsc::device_count_raw;
using tcsc::DeviceGuard;
using tcsc::hip_fail;
using tcsc::kMaxLaunchRows;
using tcsc::kUnbounded;
using tcsc::Route;
using tcsc::route_call;
using tcsc::RoutePins;
using tcsc::set_error;
using tcsc::sgemm_ws;

// RAII device allocation
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) {
        return hipMalloc(&p, bytes ? bytes : 4);
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// a plan under construction: released through tcsc_gpu_plan_destroy, so an
// early error return frees what was already allocated
struct PlanDeleter {
    void operator()(tcsc_gpu_plan* p) const { tcsc_gpu_plan_destroy(p); }
};

// Build a plan from device-resident TCSC arrays (absolute offsets).
int build_plan(int rows, int col_begin, int ncols, long long n_pos, long long n_neg, const int* csp,
               const int* csn, const int* rip, const int* rin, int device, hipStream_t st,
               tcsc_gpu_plan** out) {
    std::unique_ptr<tcsc_gpu_plan, PlanDeleter> plan(new tcsc_gpu_plan());
    plan->device = device;
    plan->rows = rows;
    plan->cols = ncols;
    plan->col_begin = col_begin;
    plan->n_pos = n_pos;
    plan->n_neg = n_neg;
    plan->n_chunks = rows > 0 ? (rows + tcsc::kTK - 1) / tcsc::kTK : 0;
    plan->n_groups = tcsc::groups_for(ncols);
    const int nch = plan->n_chunks, G = plan->n_groups;
    const long long nc = (long long)nch * ncols, ng = (long long)nch * G;
    if (n_pos + n_neg > 0x3fffffffLL || nc + 1 > 0x7fffffffLL || ng + 1 > 0x7fffffffLL) {
        set_error("plan too large: nnz=%lld buckets=%lld", n_pos + n_neg, nc);
        return TCSC_E_ARG;
    }
    HIP_TRY(hipMalloc(&plan->sptr, (size_t)(ng + 1) * sizeof(int)));
    if (ng == 0) {
        HIP_TRY(hipMemsetAsync(plan->sptr, 0, sizeof(int), st));
        HIP_TRY(hipMalloc(&plan->ent, tcsc::kEntGuard * sizeof(int2)));
        HIP_TRY(hipMemsetAsync(plan->ent, 0, tcsc::kEntGuard * sizeof(int2), st));
        HIP_TRY(hipStreamSynchronize(st));
        plan->bytes = sizeof(int) + tcsc::kEntGuard * sizeof(int2);
        *out = plan.release();
        return TCSC_OK;
    }
    tcsc::PlanDev in;
    in.rows = rows;
    in.ncols = ncols;
    in.col_begin = col_begin;
    in.n_pos = n_pos;
    in.n_neg = n_neg;
    in.csp = csp;
    in.csn = csn;
    in.rip = rip;
    in.rin = rin;
    tcsc::PlanOut po;
    po.n_chunks = nch;
    po.n_groups = G;
    po.sptr = plan->sptr;
    DevBuf lbp, lbn, cnt, cptr, gcnt, tmp, ent;
    const size_t nbnd = (size_t)(nch + 1) * ncols;
    HIP_TRY(lbp.alloc(nbnd * sizeof(int)));
    HIP_TRY(lbn.alloc(nbnd * sizeof(int)));
    HIP_TRY(cnt.alloc((size_t)(nc + 1) * sizeof(int)));
    HIP_TRY(cptr.alloc((size_t)(nc + 1) * sizeof(int)));
    HIP_TRY(gcnt.alloc((size_t)(ng + 1) * sizeof(int)));
    HIP_TRY(hipMemsetAsync(cnt.as<int>() + nc, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(gcnt.as<int>() + ng, 0, sizeof(int), st));
    size_t tb1 = 0, tb2 = 0;
    HIP_TRY(tcsc::plan_scan_tmp_bytes(nc + 1, &tb1));
    HIP_TRY(tcsc::plan_scan_tmp_bytes(ng + 1, &tb2));
    HIP_TRY(tmp.alloc(tb1 > tb2 ? tb1 : tb2));
    po.lbp = lbp.as<int>();
    po.lbn = lbn.as<int>();
    po.cnt = cnt.as<int>();
    po.cptr = cptr.as<int>();
    po.gcnt = gcnt.as<int>();
    po.scan_tmp = tmp.p;
    po.scan_tmp_bytes = tb1 > tb2 ? tb1 : tb2;
    HIP_TRY(tcsc::plan_counts(in, po, st));
    int total = 0;
    HIP_TRY(hipMemcpyAsync(&total, plan->sptr + ng, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    po.n_entries = total;
    plan->n_entries = total;
    HIP_TRY(hipMalloc(&plan->ent, (size_t)(total + tcsc::kEntGuard) * sizeof(int2)));
    po.ent = plan->ent;
    HIP_TRY(tcsc::plan_fill(in, po, st));
    HIP_TRY(hipStreamSynchronize(st));
    plan->bytes = (size_t)(ng + 1) * sizeof(int) + (size_t)(total + tcsc::kEntGuard) * sizeof(int2);
    *out = plan.release();
    return TCSC_OK;
}

// Process-wide summation order for plans created from now on
// (tcsc_gpu_set_order); initialised from $TCSC_ORDER ("reference" or "fast").
std::mutex g_order_mu;
int g_order = -1;

}  // namespace

int tcsc::current_order() {
    std::lock_guard<std::mutex> lk(g_order_mu);
    if (g_order < 0) {
        const char* e = std::getenv("TCSC_ORDER");
        g_order = (e && std::strcmp(e, "reference") == 0) ? TCSC_ORDER_REFERENCE : TCSC_ORDER_FAST;
    }
    return g_order;
}

namespace {

// ---- MFMA path selection ----------------------------------
// $TCSC_PATH at plan creation: "gather" never builds the MFMA image, "mfma"
// builds it for any W and uses it for every M, anything else (default)
// builds it when the density reaches kMfmaDensity, and a launch with
// M >= kMfmaMinM takes it where mfma_cheaper() says the GEMM is faster.
// Measured crossover (round 6, tools/crossover.py, profiles/r06_crossover.txt):
// at M = 2048 / 4096 the GEMM wins from density ~0.08; at M <= 256 (K = N =
// 8192) the unsplit GEMM, whose small grid walked all of K per workgroup,
// only from ~0.25, and since k_gemm3 splits K over such grids from ~0.04-0.1
// (profiles/r06_crossover_split.txt).  The image is built from density 0.055
// (the 0.05 configs, cfg 2/3, stay image-free; a sweep point at 0.06 is not
// lost to sampling noise under the threshold) and the choice is made per
// launch by the cost model below, fitted to those measurements.
constexpr double kMfmaDensity = 0.055;
// M <= 4 belongs to the small-M path; from 5 rows on the GEMM's 64 x 256
// tiles (M <= 64) beat the gather's 256-row tiles wherever the image exists
// (M = 8 .. 32, K = N = 8192: 1.7-5.3x, profiles/r06_mfma_narrow.txt)
constexpr int kMfmaMinM = 5;
constexpr double kMfmaMaxImageBytes = 16.0 * (1ull << 30);  // build: fp32 scratch + the bf16 W^T, 6 B a cell

int path_mode() {  // 0 auto, 1 gather only, 2 mfma forced
    const char* e = std::getenv("TCSC_PATH");
    if (!e) return 0;
    if (std::strcmp(e, "gather") == 0) return 1;
    if (std::strcmp(e, "mfma") == 0) return 2;
    return 0;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// What the fp32, bf16 and int8 calls differ in on the host, indexed by the
// activation type (tcsc::kF32 / kBf16 / kI8); everything below that routes,
// sizes or stages a call reads it from here.  The kernels' side is XSrc
// (tcsc_xsrc.h).
using tcsc::kBf16;
using tcsc::kF32;
using tcsc::kI8;
using tcsc::kYBf16;
using tcsc::kYF32;
using tcsc::Call;
using tcsc::I8Epi;
using tcsc::make_call;
using tcsc::RmsNorm;
using tcsc::YOut;
struct XType {
    const char* sgemm;  // the entry point, as error messages name it
    size_t elem;        // bytes of one element of X
    // MFMA path: the packed X (X3: [h | m | l] blocks of bf16; X1: the bf16 row;
    // X8: the int8 row) is M rows of ldx(K) elements of pack_elem bytes, W's
    // image has rows of ldw(K) elements
    int (*ldx)(int K);
    size_t pack_elem;
    int (*ldw)(int K);
    bool flags;  // the pack flags the rows its format cannot carry and a fixup recomputes them
    int (*slices)(int M, int N, int K);  // the GEMM's K split
    size_t slab_elem;                    // bytes of one element of its split-K slabs
    // cost model of the GEMM (mfma_cheaper): ops per (m, k, n), ops per
    // microsecond, microseconds per k of one workgroup's K walk
    double ops, rate, walk_us;
};
// fp32: the bf16 x3 GEMM's 6 flops per (m, k, n) at ~1.5 PFLOP/s, ~24 ns per k.
// bf16: one part instead of three -- 2 flops, a third of the sub-steps in the
// walk (~8.1 ns per k); derived from the fp32 fit, checked against
// tools/crossover.py --dtype bf16.  int8: 2 ops at twice the
// bf16 rate (v_mfma_i32_16x16x64_i8) and half the bf16 sub-steps per k (128-k
// blocks: ~4.1 ns per k), with the int8 GEMM's own K split; checked against
// tools/crossover.py --dtype i8.
constexpr XType kXTypes[3] = {
    // sgemm, elem, ldx, pack_elem, ldw, flags, slices, slab_elem, ops, rate, walk_us
    {"tcsc_gpu_sgemm", 4, tcsc::mfma_ldk, 2, tcsc::mfma_ldw, true, tcsc::mfma_slices, 4, 6.0, 1.5e9, 0.0244},
    {"tcsc_gpu_sgemm_bf16", 2, tcsc::mfma_ldw, 2, tcsc::mfma_ldw, true, tcsc::mfma_slices, 4, 2.0, 1.5e9,
     0.0244 / 3.0},
    {"tcsc_gpu_sgemm_i8", 1, tcsc::mfma8_ldw, 1, tcsc::mfma8_ldw, false, tcsc::mfma8_slices, 4, 2.0, 3.0e9,
     0.0244 / 6.0},
};

// Workspace of one MFMA launch: [packed X][M row flags, where the type keeps
// them][split-K slabs of a small grid (XType::slices; none for big tiles)],
// each part rounded up to 256 bytes.
// The bf16 call's never exceeds the fp32 call's (X1 is a third of X3, the rest
// is the same), and neither does the int8 call's, for every M, K, N:
//   * mfma8_ldw(K) = 128 ceil(K / 128) <= 128 ceil(K / 64) <= 384 ceil(K / 64) =
//     2 mfma_ldk(K) bytes, and align256 is monotone, so int8's slabs_off <=
//     fp32's flags_off <= fp32's slabs_off;
//   * mfma8_slices <= mfma_slices by construction (tcsc_mfma.hip) and both
//     slabs hold 4 B per element, so int8's slabs are no larger.
// So tcsc_gpu_plan_workspace and tcsc_gpu_plan_reserve, which size the MFMA
// path for fp32, cover bf16 and int8 launches as they are (tests/test_i8_api.py
// sweeps the inequality).
struct MfmaWs {
    size_t flags_off, slabs_off, bytes;
};
MfmaWs mfma_ws(int dt, int M, int K, int N) {
    const XType& d = kXTypes[dt];
    MfmaWs w;
    w.flags_off = align256((size_t)M * d.ldx(K) * d.pack_elem);
    w.slabs_off = w.flags_off + (d.flags ? align256((size_t)M * sizeof(int)) : 0);
    const int s = d.slices(M, N, K);
    w.bytes = w.slabs_off + (s > 1 ? (size_t)s * M * N * d.slab_elem : 0);
    return w;
}

// Variants 0-4 are the tcsc_sgemm_* family (sparse/tcsc.h); 5 is
// SparseGEMM.h's sparseGEMM<float> (bias last, no activation).  Bias first
// only for tcsc_sgemm_basic (tcsc.c:74-96).
bool valid_variant(int v) { return v >= TCSC_VARIANT_BASIC && v <= TCSC_VARIANT_SPARSE_GEMM; }
bool is_prelu(int v) { return v >= TCSC_VARIANT_PRELU_BASIC && v <= TCSC_VARIANT_PRELU_ONTHEGO; }

// Per-launch cost model (microseconds), fitted to tools/crossover.py on the
// box (profiles/r06_crossover_split.txt, r06_crossover_small.txt: 120
// shapes x densities, M = 64 .. 4096, K and N = 256 .. 8192):
//  * gather: ~38 us fixed + one add per nonzero and row of the 256-row tiles
//    it runs (M rounded up to 256) at ~23 T adds/s;
//  * MFMA: ~10 us fixed (k_split3, k_fixup, launches) + the larger of the
//    GEMM's ops per (m, k, n) at its rate (XType: fp32's bf16 x3 GEMM is 6
//    flops at ~1.5 PFLOP/s) and the K walk of one workgroup (fp32 ~24 ns per
//    k, the slice's share when K is split; x1.5 with two workgroups per CU),
//    + for a split K the slab reduce (~3 us + the slabs read and Y written at
//    ~4 TB/s).
// With these constants the default plan is within 1.02x of the faster
// forced path at every measured point.  The gather term, the fixed cost and
// the reduce are the same for every activation type (only the gather's
// transpose reads less).
bool mfma_cheaper(const tcsc_gpu_plan* p, int M, int dt) {
    const XType& d = kXTypes[dt];
    const double nnz = (double)(p->n_pos + p->n_neg), Kb = (double)d.ldw(p->rows);
    const double Mp = (double)(((long long)M + tcsc::kTM - 1) / tcsc::kTM * tcsc::kTM);
    const double gather_us = 38.0 + Mp * nnz / 23.0e6;
    const int s = d.slices(M, p->cols, p->rows);
    const double walk_us = Kb * d.walk_us / s * (tcsc::mfma_tiles(M, p->cols) * s > 256 ? 1.5 : 1.0);
    const double reduce_us = s > 1 ? 3.0 + (s + 1.0) * M * p->cols * 4.0 / 4.0e6 : 0.0;
    const double mfma_us = 10.0 + std::max(d.ops * M * Kb * p->cols / d.rate, walk_us) + reduce_us;
    return mfma_us < gather_us;
}

// forced (TCSC_PATH=mfma: mfma_min_M 1): every launch; default: by the cost
// model.  An int8 call needs the int8 image (tcsc_gpu_plan_enable_i8).
bool has_mfma(const tcsc_gpu_plan* p, int M, int dt) {  // the plan can run M rows of type dt on the MFMA path
    if (p->packed) return dt == kI8 && p->w2 && M >= p->mfma_min_M && p->rows > 0;  // k_gemm8w2 on the 2-bit image
    return p->wt && (dt != kI8 || p->w8) && M >= p->mfma_min_M && p->rows > 0;
}
bool use_mfma(const tcsc_gpu_plan* p, int M, int dt = kF32) {
    if (!has_mfma(p, M, dt)) return false;
    if (p->mfma_min_M == 1 || p->packed) return true;  // forced, or the only path the plan has at this M
    return mfma_cheaper(p, M, dt);
}

rocblas_handle rocblas_for_device(int dev) {
    static std::mutex mu;
    static std::unordered_map<int, rocblas_handle> handles;
    std::lock_guard<std::mutex> lk(mu);
    auto it = handles.find(dev);
    if (it != handles.end()) return it->second;
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != rocblas_status_success) return nullptr;
    handles[dev] = h;
    return h;
}

void free_w2(tcsc_gpu_plan* p) {
    if (p->w2) (void)hipFree(p->w2);
    p->w2 = nullptr;
    p->w2_bytes = 0;
}

void free_i8(tcsc_gpu_plan* p) {
    free_w2(p);  // made from the int8 image, useless without it
    if (p->w8) (void)hipFree(p->w8);
    p->w8 = nullptr;
    p->i8_bytes = 0;
}

void free_mfma(tcsc_gpu_plan* p) {
    free_i8(p);  // made from the bf16 image, useless without it
    if (p->wt) (void)hipFree(p->wt);
    p->wt = nullptr;
    p->mfma_bytes = 0;
}

void free_csc(tcsc_gpu_plan* p) {
    for (void* q : {(void*)p->ccq, (void*)p->crq})
        if (q) (void)hipFree(q);
    p->ccq = p->crq = nullptr;
    p->csc_bytes = 0;
}

// Whether maybe_build_mfma would build the MFMA image for this plan (before
// the allocation and bf16-exactness checks): the path mode, the image's size
// and K limits and, by default, the density threshold.
bool mfma_wanted(const tcsc_gpu_plan* p, bool allow_mfma) {
    const int mode = path_mode();
    const double cells = (double)p->rows * p->cols;
    const long long nnz = p->n_pos + p->n_neg;
    if (!allow_mfma || mode == 1 || cells == 0 || 6.0 * cells > kMfmaMaxImageBytes) return false;
    // k_gemm3's DMA offsets are 32-bit bytes within a 256-row tile: K < ~2.8 M
    if (512.0 * tcsc::mfma_ldk(p->rows) >= 4294967296.0) return false;
    return !(mode == 0 && (nnz < kMfmaDensity * cells || p->rows < 64 || p->cols < 64));
}

// The merged CSC copy of a fast-order plan's column range (the quad layout of
// tcsc_internal.h: one 4-byte entry per nonzero, each 64-column group padded
// to its longest column, plus 4 bytes per group).  Only its two consumers
// want it: the small-M path (K small enough for X to fit the LDS) and the
// MFMA path's fixup.  A group padded far past its nonzeros (a few long
// columns among short ones) is not worth its memory: above kCscMaxPad times
// the nonzeros the copy is dropped.  Not building it is not an error: the
// small-M path and the MFMA path are then off for this plan.
constexpr double kCscMaxPad = 4.0;
int build_csc(tcsc_gpu_plan* p, const int* csp, const int* csn, const int* rip, const int* rin, int col_begin,
              bool allow_mfma, hipStream_t st) {
    // entries are byte offsets 4*k (+1 rows) and 4*Kp + 4*k (-1 rows), Kp = K + 1
    // rounded up to 4: below 2^31 while K < 2^27 - 4
    if (p->cols == 0 || p->rows >= (1 << 27) - 4) return TCSC_OK;
    if (!tcsc::small_m_fits(1, p->rows) && !mfma_wanted(p, allow_mfma)) return TCSC_OK;
    const int nc = p->cols, ng = tcsc::csc_groups(nc);
    size_t tb = 0;
    DevBuf tcp, tcn, trp, trn, gq, tmp;  // scratch: the rebased per-sign lists, merged into crq
    if (tcsc::plan_scan_tmp_bytes(ng + 1, &tb) != hipSuccess || hipMalloc(&p->ccq, (size_t)(ng + 1) * sizeof(int)) != hipSuccess ||
        tcp.alloc((size_t)(nc + 1) * sizeof(int)) != hipSuccess || tcn.alloc((size_t)(nc + 1) * sizeof(int)) != hipSuccess ||
        gq.alloc((size_t)(ng + 1) * sizeof(int)) != hipSuccess || tmp.alloc(tb) != hipSuccess ||
        trp.alloc((size_t)(p->n_pos > 0 ? p->n_pos : 1) * sizeof(int)) != hipSuccess ||
        trn.alloc((size_t)(p->n_neg > 0 ? p->n_neg : 1) * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        free_csc(p);
        return TCSC_OK;
    }
    HIP_TRY(tcsc::csc_prepare(csp, csn, rip, rin, col_begin, nc, p->n_pos, p->n_neg, tcp.as<int>(), tcn.as<int>(),
                              trp.as<int>(), trn.as<int>(), gq.as<int>(), tmp.p, tb, p->ccq, st));
    int quads = 0;
    HIP_TRY(hipMemcpyAsync(&quads, p->ccq + ng, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t ent = tcsc::csc_quad_entries(quads);
    const double nnz = (double)(p->n_pos + p->n_neg);
    if ((double)ent > kCscMaxPad * nnz + (double)tcsc::csc_quad_entries(16LL * ng)) {
        free_csc(p);  // padding-dominated: gather only
        return TCSC_OK;
    }
    if (hipMalloc(&p->crq, ent * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        free_csc(p);
        return TCSC_OK;
    }
    p->csc_bytes = (size_t)(ng + 1) * sizeof(int) + ent * sizeof(int);
    HIP_TRY(tcsc::csc_fill(tcp.as<int>(), tcn.as<int>(), trp.as<int>(), trn.as<int>(), p->ccq, nc, p->rows, p->crq,
                           ent, st));
    HIP_TRY(hipStreamSynchronize(st));  // the scratch is freed on return
    return TCSC_OK;
}

// Small-M path (tcsc_small.hip) on fast-order plans: M <= 4 rows whose X and
// -X fit the LDS, one lane per output column.  The gather costs the same
// ~256-row tile for any M <= 256 plus ~20 us of staging and launch; the small
// path's cost grows with M * nnz.  Measured on one box (tools/r5_small.sh,
// prelu_basic, small vs gather): 1 x 512 x 2048 7.9 vs 36.8 us, 1 x 2048 x
// 8192 16.1 vs 111 us, 1 x 16384^2 15.0 vs 93 us, 4 x 4096^2 15.1 vs 36.4 us.
// M = 4 at K = 16384 does not fit the LDS and stays on the gather.
// $TCSC_SMALL_M caps M (0 = off).
constexpr int kSmallMaxM = 4;
int small_max_m() {
    const char* e = std::getenv("TCSC_SMALL_M");
    if (!e) return kSmallMaxM;
    return std::max(0, std::min(kSmallMaxM, std::atoi(e)));
}

bool has_small(const tcsc_gpu_plan* p, int M) {  // the plan can run M rows on the small-M path
    return p->crq && p->rows > 0 && M >= 1 && M <= small_max_m() && tcsc::small_m_fits(M, p->rows);
}
bool use_small(const tcsc_gpu_plan* p, int M, int dt = kF32) { return has_small(p, M) && !use_mfma(p, M, dt); }

// The decode path (tcsc_decode.hip): int8 calls of M <= 16 rows
// on a plan with the 2-bit image.  The default rule compares the bytes of W a
// call reads: above 4 rows the alternative is k_gemm8 on the int8 image, 1 byte
// per weight against a quarter; up to 4 rows it is k_small_m on the merged CSC
// copy, 4 bytes per nonzero against a quarter byte per weight -- unless X does
// not fit the small-M path's LDS, which leaves k_gemm8 or the gather.
bool decode_pays(int M, int K, int N, long long nnz) {
    if (M < 1 || M > tcsc::kDecodeMaxM) return false;
    return M > kSmallMaxM || !tcsc::small_m_fits(M, K) || 16 * nnz > (long long)K * N;
}
// $TCSC_DECODE, read per call: 0 never, 1 at every M <= 16 where the image exists, unset the rule
int decode_knob() {
    const char* e = std::getenv("TCSC_DECODE");
    if (!e || !*e) return -1;
    return std::atoi(e) != 0 ? 1 : 0;
}
// $TCSC_W2GEMM=1, read per call: int8 calls that route to TCSC_PATH_MFMA on an ordinary plan with the 2-bit
// image run k_gemm8w2 instead of k_gemm8 (the A/B on one plan); never a default
bool w2gemm_knob() {
    const char* e = std::getenv("TCSC_W2GEMM");
    return e && std::atoi(e) != 0;
}
// The row-tiled launches (k_decode8r): where one launch of 16 < M <= 64 rows beats k_pack8 +
// k_gemm8w2, fitted to profiles/decode_rows_bench.json: 1 for 17 <= M <= 32 and K N <= 2^26.  With two row
// tiles the launch beat the GEMM beyond the run's spread at every measured point (five shapes from 2560^2 to
// 8192^2, M = 17, 24, 32: 1.23x to 2.23x).  With four (M >= 33) it won at 2560^2, 4096^2 and 8192^2 and lost
// at 2560 x 6912 and 6912 x 2560 (0.83x to 0.98x), and nothing monotone in M, K, N and the CU count separates
// those, so the rule is 0 from 33 rows on.  K N <= 2^26 is the largest shape measured (the margin falls with
// the size of W: 2.2x at 2560^2, 1.23x at 8192^2, M = 32); below the smallest the GEMM's two launches cost 11 us
// whatever the shape and the one decode launch less than half of it.  num_cus does not enter.
constexpr long long kDecodeRowsMaxKN = 1LL << 26;
constexpr int kDecodeRowsPaysM = 32;
bool decode_rows_pays(int M, int K, int N, int num_cus) {
    (void)num_cus;
    if (M <= tcsc::kDecodeMaxM || M > kDecodeRowsPaysM || K < 1 || K >= tcsc::kDecodeMaxK || N < 1) return false;
    return (long long)K * N <= kDecodeRowsMaxKN;
}
// the plan's setting admits M rows (M > 16) to the decode path
bool decode_rows_on(const tcsc_gpu_plan* p, int M) {
    if (M <= tcsc::kDecodeMaxM || M > tcsc::kDecodeRowsMax) return false;
    if (p->decode_rows == TCSC_DECODE_ROWS_AUTO) return decode_rows_pays(M, p->rows, p->cols, p->num_cus);
    return M <= p->decode_rows;
}
// The gated and grouped row-tiled launches (k_decode8gr / k_decode8mr): where the one launch of
// 16 < M <= 64 rows beats k_pack8 + one k_gemm8w2 per matrix, fitted to profiles/multi_rows_bench.json
// (tools/multi_rows_bench.py) and to nothing else.  The one launch beat both samples of the parent at all 36
// measured points of 17 .. 64 rows, with two row tiles and with four: the gated call 1.15x to 2.40x (2560 x 6912,
// 4096^2, 8192^2), the grouped one 1.19x to 3.45x (2560: 2560 + 640 + 640, 4096: 3 x 4096, 8192: 8192 + 1024 + 1024).
// The margin falls with the size of W and with M (8192^2 at M = 64: 1.15x; 8192 x 10240 at M = 64: 1.19x), so each rule
// stops at the largest shape measured: gated 1 for 17 <= M <= 64 and K H <= 2^26, grouped 1 for 17 <= M <= 64 and
// K (sum of the members' columns) <= 8192 * 10240.  Below the smallest shape measured the MFMA route's launches cost
// 25 us (gated) and 32 us (grouped) whatever the shape and the one decode launch 9 to 15 us.  num_cus does not enter.
constexpr long long kGluRowsMaxKH = 1LL << 26;
constexpr long long kGroupRowsMaxKN = 8192LL * 10240LL;
bool glu_rows_pays(int M, int K, int H, int num_cus) {
    (void)num_cus;
    if (M <= tcsc::kDecodeMaxM || M > tcsc::kDecodeRowsMax || K < 1 || K >= tcsc::kDecodeMaxK || H < 1) return false;
    return (long long)K * H <= kGluRowsMaxKH;
}
bool group_rows_pays(int M, int K, const int* cols, int count, int num_cus) {
    (void)num_cus;
    if (M <= tcsc::kDecodeMaxM || M > tcsc::kDecodeRowsMax || K < 1 || K >= tcsc::kDecodeMaxK || !cols || count < 1 ||
        count > tcsc::kGroupMax)
        return false;
    long long total = 0;
    for (int i = 0; i < count; ++i) {
        if (cols[i] < 1) return false;
        total += cols[i];
    }
    return (long long)K * total <= kGroupRowsMaxKN;
}
// the plan's decode_rows_multi setting admits M rows (M > 16); `pays` is the call's own rule, asked under AUTO
bool multi_rows_admits(const tcsc_gpu_plan* p, int M, bool pays) {
    if (M <= tcsc::kDecodeMaxM || M > tcsc::kDecodeRowsMax) return false;
    if (p->decode_rows_multi == TCSC_DECODE_ROWS_AUTO) return pays;
    return M <= p->decode_rows_multi;
}
// a gated call of M rows takes TCSC_PATH_DECODE: up to 16 rows always, above where gate and up admit M
bool glu_decodes(const tcsc_gpu_plan* gate, const tcsc_gpu_plan* up, int M) {
    if (M <= tcsc::kDecodeMaxM) return true;
    if (M > tcsc::kDecodeRowsMax) return false;
    const bool pays = glu_rows_pays(M, gate->rows, gate->cols, gate->num_cus);
    return multi_rows_admits(gate, M, pays) && multi_rows_admits(up, M, pays);
}
bool has_decode(const tcsc_gpu_plan* p, int M, int dt) {  // the plan can run M rows of type dt on the decode path
    return dt == kI8 && p->w2 && M >= 1 && (M <= tcsc::kDecodeMaxM || decode_rows_on(p, M));
}
bool use_decode(const tcsc_gpu_plan* p, int M, int dt) {
    if (!has_decode(p, M, dt)) return false;
    if (p->packed) return true;  // nothing else serves M <= 16 there: neither the rule nor $TCSC_DECODE is asked
    const int knob = decode_knob();
    if (M > tcsc::kDecodeMaxM) return knob != 0;  // the plan's setting decides; $TCSC_DECODE=0 still vetoes
    return knob >= 0 ? knob == 1 : decode_pays(M, p->rows, p->cols, p->n_pos + p->n_neg);
}

// Adds the MFMA image to a fast-order plan when the path mode and the density
// call for it.  Not building it is never an error: the gather serves every M.
int maybe_build_mfma(tcsc_gpu_plan* p, const int* csp, const int* csn, const int* rip, const int* rin, int col_begin,
                     bool allow_mfma, hipStream_t st) {
    const int mode = path_mode();
    if (!mfma_wanted(p, allow_mfma)) return TCSC_OK;
    if (!p->crq) return TCSC_OK;  // the fixup needs the CSC copy
    const size_t n = (size_t)p->rows * p->cols;
    DevBuf wf, bad;
    if (wf.alloc(n * sizeof(float)) != hipSuccess || bad.alloc(sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        return TCSC_OK;  // no room for the image: gather only
    }
    const int ldw = tcsc::mfma_ldw(p->rows);
    const size_t wtb = (size_t)p->cols * ldw * sizeof(uint16_t);
    if (hipMalloc(&p->wt, wtb) != hipSuccess) {
        (void)hipGetLastError();
        free_mfma(p);
        return TCSC_OK;
    }
    p->mfma_bytes = wtb;
    HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int), st));
    HIP_TRY(tcsc::mfma_build_wt(csp, csn, rip, rin, col_begin, p->rows, p->cols, wf.as<float>(), p->wt, ldw,
                                p->n_pos, p->n_neg, bad.as<int>(), st));
    int hbad = 0;
    HIP_TRY(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hbad) free_mfma(p);  // a column repeats a row > 256 times: not exact in bf16
    p->mfma_min_M = mode == 2 ? 1 : kMfmaMinM;
    return TCSC_OK;
}

// The plan, plus -- in reference order -- its two one-sign chains: the same
// build on the same arrays with the other sign's col_start replaced by zeros.
// allow_mfma false: never the MFMA image (the host API's exact mode).
int build_plan_ordered(int rows, int col_begin, int ncols, long long n_pos, long long n_neg, const int* csp,
                       const int* csn, const int* rip, const int* rin, int device, hipStream_t st, int order,
                       tcsc_gpu_plan** out, bool allow_mfma = true) {
    int rc = build_plan(rows, col_begin, ncols, n_pos, n_neg, csp, csn, rip, rin, device, st, out);
    if (rc != TCSC_OK) return rc;
    if (order != TCSC_ORDER_REFERENCE) {
        rc = build_csc(*out, csp, csn, rip, rin, col_begin, allow_mfma, st);
        if (rc == TCSC_OK) rc = maybe_build_mfma(*out, csp, csn, rip, rin, col_begin, allow_mfma, st);
        if (rc != TCSC_OK) {
            tcsc_gpu_plan_destroy(*out);
            *out = nullptr;
        }
        return rc;
    }
    tcsc_gpu_plan* p = *out;
    p->order = order;
    DevBuf zeros;
    const size_t zb = (size_t)(col_begin + ncols + 1) * sizeof(int);
    if (zeros.alloc(zb) != hipSuccess || hipMemsetAsync(zeros.p, 0, zb, st) != hipSuccess) {
        tcsc_gpu_plan_destroy(p);
        *out = nullptr;
        set_error("tcsc_gpu_plan_create: cannot allocate the reference-order chains");
        return TCSC_E_HIP;
    }
    rc = build_plan(rows, col_begin, ncols, n_pos, 0, csp, zeros.as<int>(), rip, rip, device, st, &p->chain_pos);
    if (rc == TCSC_OK)
        rc = build_plan(rows, col_begin, ncols, 0, n_neg, zeros.as<int>(), csn, rin, rin, device, st, &p->chain_neg);
    if (rc != TCSC_OK) {
        tcsc_gpu_plan_destroy(p);
        *out = nullptr;
    }
    return rc;
}

// TCSC_SLICES=n forces the split-K factor (tests, tuning); read per call.
int slices_override() {
    const char* s = std::getenv("TCSC_SLICES");
    return s ? std::atoi(s) : 0;
}

// TCSC_COMBINE_GIVEUP=1 (tests): in the in-launch combine every slice of a
// tile except the last to arrive stops waiting at once, so the last arrival
// reduces every band (the path a non-resident slice would take)
int combine_giveup_knob() {
    const char* s = std::getenv("TCSC_COMBINE_GIVEUP");
    return s && std::atoi(s) != 0 ? 1 : 0;
}

// Workspace of one fp32 call on each path, whatever the cost model prefers at
// this M; 0 where the plan cannot run the path (tcsc_gpu_plan_workspace).
size_t path_ws_bytes(const tcsc_gpu_plan* p, int M, int path) {
    if (M <= 0 || p->cols == 0) return 0;
    RoutePins pin;
    pin.path = path;
    return route_call(p, M, p->packed ? kI8 : kF32, kUnbounded, pin).ws_bytes;  // a packed plan runs int8 calls only
}

// the path of a call of type dt (each type has its own cost model)
int launch_path(const tcsc_gpu_plan* p, int M, int dt = kF32) {
    if (use_decode(p, M, dt)) return TCSC_PATH_DECODE;
    return use_mfma(p, M, dt) ? TCSC_PATH_MFMA : use_small(p, M, dt) ? TCSC_PATH_SMALL : TCSC_PATH_GATHER;
}

// Workspace of the call of type dt at this M, on the path it takes.
size_t wanted_workspace(const tcsc_gpu_plan* p, int M, int dt = kF32) {
    if (M <= 0 || p->cols == 0) return 0;
    return route_call(p, M, dt, kUnbounded, RoutePins()).ws_bytes;
}

// tcsc_gpu_plan_reserve(max_M): the largest need of any M <= max_M on any path
// the plan has.  Neither need grows with M: both cost models split K more at
// smaller M (fewer row tiles to fill the CUs), so slices x M x N peaks inside
// the range -- K = 512, N = 4096 at 2 % wants 14x more at M = 339 than at 512.
// So every M is evaluated (16 cost-model steps each) up to the row count from
// which the answer is known:
//  * gather: choose_slices takes s > 1 only where t(s) < 0.97 t(1); t(s) is at
//    least base nch / 256 chunk times (base = row tiles x column blocks) and
//    t(1) is ceil(base / 256) nch of them, so from base = 8278 on nothing is
//    split (kNoSplitBase adds a margin for the rounding of the doubles) and
//    the need is xt_bytes(M), which grows with M; a forced split
//    ($TCSC_SLICES) is the same for every M and its need grows with M too;
//  * MFMA: the slice count changes only where a tile count does, at multiples
//    of 64 rows, and between those the need grows with M: the top row of every
//    64-row step is evaluated (one division each);
// and max_M itself.
constexpr long long kNoSplitBase = 40 * 256;
size_t reserve_bytes(const tcsc_gpu_plan* p, int max_M) {
    if (max_M <= 0 || p->cols == 0) return 0;
    if (p->packed) {  // the MFMA rule below is all there is: X8 and the i32 slabs of k_gemm8w2 (k_decode8 needs nothing)
        const int top = std::min(max_M, kMaxLaunchRows);
        size_t want = path_ws_bytes(p, top, TCSC_PATH_MFMA);
        for (int M = 64; M < top; M += 64) want = std::max(want, path_ws_bytes(p, M, TCSC_PATH_MFMA));
        return want;
    }
    const long long cb = std::max(1, (p->n_groups + tcsc::kWaves - 1) / tcsc::kWaves);
    const int every = (int)std::min<long long>(max_M, (kNoSplitBase + cb - 1) / cb * tcsc::kTM);
    size_t want = 0;
    auto all_paths = [&](int M) {
        for (int path : {TCSC_PATH_GATHER, TCSC_PATH_MFMA, TCSC_PATH_SMALL})
            want = std::max(want, path_ws_bytes(p, M, path));
    };
    for (int M = 1; M <= every; ++M) all_paths(M);
    if (p->wt)
        for (long long M = ((long long)every / 64 + 1) * 64; M < max_M; M += 64)
            want = std::max(want, path_ws_bytes(p, (int)M, TCSC_PATH_MFMA));
    all_paths(max_M);
    return want;
}

// The plan build assumes what tcsc_from_dense produces (tcsc.c:48-60): in
// every column the row indices lie in [0, rows) and ascend.  The reference's
// loops take any order (tcsc.c:86-93), so a column out of order is sorted in
// a copy (its sums then run in ascending k: within the float tolerance of
// the reference's order, exact on integer-valued inputs).  A row outside
// [0, rows) or a decreasing col_start would make the reference read outside
// X or the index arrays: TCSC_E_ARG.  Columns [c0, c1) of one sign; on
// return `sorted` is empty when the slice is already in order, else the
// whole slice (rebased to cs[c0]) with every column sorted.
int check_index_host(const int* cs, const int* ri, int c0, int c1, int rows, int n_elem, const char* sign,
                     std::vector<int>& sorted) {
    sorted.clear();
    bool in_order = true;
    for (int j = c0; j < c1; ++j) {
        const int a = cs[j], b = cs[j + 1];
        if (a < 0 || b < a || b > n_elem) {
            set_error("tcsc_gpu_plan_create: col_start_%s[%d..%d] = %d, %d is not a range inside [0, %d]", sign, j,
                      j + 1, a, b, n_elem);
            return TCSC_E_ARG;
        }
        for (int i = a; i < b; ++i) {
            const int k = ri[i];
            if (k < 0 || k >= rows) {
                set_error("tcsc_gpu_plan_create: row_index_%s[%d] = %d outside [0, %d) (column %d)", sign, i, k, rows,
                          j);
                return TCSC_E_ARG;
            }
            if (i > a && k < ri[i - 1]) in_order = false;
        }
    }
    if (in_order) return TCSC_OK;
    const int base = cs[c0];
    sorted.assign(ri + base, ri + cs[c1]);
    for (int j = c0; j < c1; ++j) std::sort(sorted.begin() + (cs[j] - base), sorted.begin() + (cs[j + 1] - base));
    return TCSC_OK;
}

}  // namespace

namespace tcsc {

// Content fingerprint of index arrays for the host API's plan cache.  The
// cache is keyed by the tcsc_t pointer, but the reference reads the arrays
// on every call and keeps no state, so an in-place rebuild with the same
// counts, or a tcsc_t released with plain free() (as the reference's
// test_bcsr.cpp does for bcsr_t) whose addresses malloc hands to the next
// matrix, must not hit a stale plan.  Multilinear hash over 32-bit pairs in
// four lanes (it vectorises: ~1 ms for cfg4's 21 MB of indices, next to the
// ~5 ms H2D of X every call pays), position-dependent, murmur-finalised.
uint64_t fmix64(uint64_t h) {
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 33);
}

constexpr uint32_t kHashA[4] = {0x9e3779b9u, 0x85ebca6bu, 0xc2b2ae35u, 0x27d4eb2fu};
constexpr uint32_t kHashB[4] = {0x165667b1u, 0xd3a2646cu, 0xfd7046c5u, 0xb55a4f09u};

// The sums over whole 8-int groups [i0, i1) (multiples of 8) into acc: a sum,
// so disjoint ranges can be summed on different threads (AsyncFingerprint).
void hash_groups(const uint32_t* u, long long i0, long long i1, uint64_t acc[4]) {
    for (long long i = i0; i < i1; i += 8) {
        const uint32_t pos = (uint32_t)i;
        for (int j = 0; j < 4; ++j)
            acc[j] += (uint64_t)(u[i + 2 * j] + kHashA[j] + pos) * (uint64_t)(u[i + 2 * j + 1] + kHashB[j]);
    }
}

// The tail (n % 8 ints) and the finalisation, given the groups' sums.
uint64_t hash_finish(const uint32_t* u, long long n, uint64_t h, uint64_t acc[4]) {
    for (long long i = n & ~7LL; i < n; ++i)
        acc[i & 3] += (uint64_t)(u[i] + kHashA[i & 3] + (uint32_t)i) * (uint64_t)(kHashB[i & 3] | 1u);
    for (int j = 0; j < 4; ++j) h = fmix64(h ^ acc[j]) + (uint64_t)j;
    return h;
}

uint64_t hash_ints(const int* p, long long n, uint64_t h) {
    h = fmix64(h ^ (uint64_t)n);
    if (!p || n <= 0) return h;
    const uint32_t* u = reinterpret_cast<const uint32_t*>(p);
    uint64_t acc[4] = {0, 0, 0, 0};
    hash_groups(u, 0, n & ~7LL, acc);
    return hash_finish(u, n, h, acc);
}

uint64_t tcsc_fingerprint(const tcsc_t* W) {
    uint64_t h = fmix64(((uint64_t)(uint32_t)W->rows << 32) | (uint32_t)W->cols);
    h = hash_ints(W->col_start_pos, (long long)W->cols + 1, h);
    h = hash_ints(W->col_start_neg, (long long)W->cols + 1, h);
    h = hash_ints(W->row_index_pos, W->n_elem_pos, h);
    return hash_ints(W->row_index_neg, W->n_elem_neg, h);
}

}  // namespace tcsc

namespace {

// ---- the two gather geometries (DESIGN.md §4 "Two geometries") --------------
// A launch of M rows over ncols columns runs ceil(M / 256) x ceil(ncols / w)
// workgroups of w columns, one per CU at a time, so it takes
//   rounds(w) = ceil(ceil(M / 256) * ceil(ncols / w) / num_cus)
// passes over the chip, each about as long as one workgroup's K walk, which
// costs in proportion to the workgroup's columns.  The 22-column geometry (w =
// 352) pays where   rounds(352) * 352 * alpha < rounds(256) * 256,
// alpha = the measured cost per column of a wide workgroup over a narrow one.
// Fitted on cfg 4, both kernels of one library alternating on one MI355X
// (profiles/wide_ab_kernels.txt, HIP events, 3 rounds): k_stream 1.1819 ms in
// 4 rounds of 256 columns, k_stream_w 1.1216 ms in 3 rounds of 352:
//   alpha = (1.1216 / (3 * 352)) / (1.1819 / (4 * 256)) = 0.920.
// Fitted at 98 % sparsity, where a wave's chunk stream (21 entries) fits the
// wide loop's 30-entry scalar buffer; denser W was not measured.
constexpr double kWideAlpha = 0.92;
bool wide_pays(int M, int ncols, int num_cus) {
    if (M <= 0 || ncols <= 0 || num_cus <= 0) return false;
    const long long rt = ((long long)M + tcsc::kTM - 1) / tcsc::kTM;
    auto rounds = [&](int w) { return (rt * ((ncols + w - 1) / w) + num_cus - 1) / num_cus; };
    return (double)(rounds(tcsc::kWideWgCols) * tcsc::kWideWgCols) * kWideAlpha <
           (double)(rounds(tcsc::kWgCols) * tcsc::kWgCols);
}

// $TCSC_GEO=16|22 forces a geometry (tests, A/B); read per call.  0: the rounds model.
int geo_override() {
    const char* s = std::getenv("TCSC_GEO");
    const int v = s ? std::atoi(s) : 0;
    return v == tcsc::kCW || v == tcsc::kWideCW ? v : 0;
}

// Whether tcsc_gpu_plan_reserve(max_M) builds the wide streams: a fast-order
// forward plan with entries whose launch of some M <= max_M would take them (the
// model is not monotone in M, so every row-tile count is asked), or $TCSC_GEO=22.
bool wide_wanted(const tcsc_gpu_plan* p, int max_M) {
    if (p->order != TCSC_ORDER_FAST || p->tbias || p->rows <= 0 || p->cols <= 0 || max_M <= 0 || !p->ent || !p->sptr)
        return false;  // the backward pass's transposed plans keep the 16-column kernel
    const int f = geo_override();
    if (f == tcsc::kWideCW) return true;
    if (f == tcsc::kCW) return false;
    const int top = std::min(max_M, kMaxLaunchRows);
    for (long long M = tcsc::kTM; M < top + tcsc::kTM; M += tcsc::kTM)
        if (wide_pays((int)std::min<long long>(M, top), p->cols, p->num_cus)) return true;
    return false;
}

// The second copy of the entry streams, from the plan's own (tcsc_wide.hip).
// Synchronises; a failure to allocate is no error (the 16-column kernel
// serves every launch).
int build_wide(tcsc_gpu_plan* p) {
    if (p->ent_w) return TCSC_OK;
    DeviceGuard dg(p->device);
    hipStream_t st = nullptr;
    const int nch = p->n_chunks, G = p->n_groups, ncols = p->cols, Gw = tcsc::wide_groups_for(ncols);
    const long long nc = (long long)nch * ncols, ng = (long long)nch * Gw;
    if (nch <= 0 || ng + 1 > 0x7fffffffLL) return TCSC_OK;
    // $TCSC_WIDE_BALANCE=0 keeps every wave on its contiguous 22 columns (the
    // identity slot map: the A/B of the balanced assignment); read here only
    const char* bal_s = std::getenv("TCSC_WIDE_BALANCE");
    const int balance = bal_s && std::atoi(bal_s) == 0 ? 0 : 1;
    const size_t nmap = (size_t)tcsc::wide_blocks_for(ncols) * tcsc::kWideWgCols;
    DevBuf cnt, cptr, gcnt, tmp, loads, winv, wstats;
    size_t tb1 = 0, tb2 = 0;
    HIP_TRY(tcsc::plan_scan_tmp_bytes(nc + 1, &tb1));
    HIP_TRY(tcsc::plan_scan_tmp_bytes(ng + 1, &tb2));
    const size_t tb = std::max(tb1, tb2);
    int* sptr_w = nullptr;
    unsigned short* wperm = nullptr;
    if (cnt.alloc((size_t)(nc + 1) * sizeof(int)) != hipSuccess || cptr.alloc((size_t)(nc + 1) * sizeof(int)) != hipSuccess ||
        gcnt.alloc((size_t)(ng + 1) * sizeof(int)) != hipSuccess || tmp.alloc(tb) != hipSuccess ||
        loads.alloc(nmap / tcsc::kWideCW * nch * sizeof(int)) != hipSuccess ||
        winv.alloc((size_t)ncols * sizeof(unsigned short)) != hipSuccess ||
        wstats.alloc(4 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&sptr_w, (size_t)(ng + 1) * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        return TCSC_OK;
    }
    std::unique_ptr<int, void (*)(int*)> sptr_guard(sptr_w, [](int* q) { (void)hipFree(q); });
    if (hipMalloc(&wperm, nmap * sizeof(unsigned short)) != hipSuccess) {
        (void)hipGetLastError();
        return TCSC_OK;
    }
    std::unique_ptr<unsigned short, void (*)(unsigned short*)> wperm_guard(wperm, [](unsigned short* q) { (void)hipFree(q); });
    HIP_TRY(hipDeviceSynchronize());  // the plan's streams are complete (built on the creator's stream)
    HIP_TRY(tcsc::wide_counts(p->ent, p->sptr, G, nch, ncols, Gw, balance, cnt.as<int>(), cptr.as<int>(), gcnt.as<int>(),
                              sptr_w, loads.as<int>(), wperm, winv.as<unsigned short>(), wstats.as<unsigned long long>(),
                              tmp.p, tb, st));
    int total = 0;
    unsigned long long stats[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&total, sptr_w + ng, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stats, wstats.p, sizeof stats, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int2* ent_w = nullptr;
    if (hipMalloc(&ent_w, (size_t)(total + tcsc::kEntGuard) * sizeof(int2)) != hipSuccess) {
        (void)hipGetLastError();
        return TCSC_OK;
    }
    hipError_t e = tcsc::wide_fill(p->ent, p->sptr, G, nch, ncols, Gw, cptr.as<int>(), winv.as<unsigned short>(), sptr_w,
                                   ent_w, total, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the scratch is freed on return
    if (e != hipSuccess) {
        (void)hipFree(ent_w);
        return hip_fail(e, "build_wide");
    }
    p->ent_w = ent_w;
    p->sptr_w = sptr_guard.release();
    p->wperm = wperm_guard.release();
    for (int i = 0; i < 4; ++i) p->wide_stats[i] = (long long)stats[i];
    p->n_entries_w = total;
    p->n_groups_w = Gw;
    p->wide_bytes = (size_t)(ng + 1) * sizeof(int) + (size_t)(total + tcsc::kEntGuard) * sizeof(int2) +
                    nmap * sizeof(unsigned short);
    return TCSC_OK;
}

// The geometry of a gather launch of M rows (kCW or kWideCW), given the K
// split it would run with the 16-column kernel (rounded to whole chunks) and
// whether the caller forces one; -1 where $TCSC_GEO=22 cannot be had, with
// the error set for a caller that names itself.
int launch_geo(const tcsc_gpu_plan* p, int M, int slices, int forced_slices, const char* who) {
    const int f = geo_override();
    if (f == tcsc::kWideCW) {
        if (p->order != TCSC_ORDER_FAST || forced_slices > 1) {
            if (who)
                set_error("%s: TCSC_GEO=22 needs the fast order and an unsplit K (order %s, %d slices forced)", who,
                          p->order == TCSC_ORDER_FAST ? "fast" : "reference", forced_slices);
            return -1;
        }
        if (p->rows <= 0) return tcsc::kCW;  // nothing to gather: the bias alone, either kernel
        if (!p->ent_w) {
            if (who)
                set_error("%s: TCSC_GEO=22 but the plan has no wide streams (tcsc_gpu_plan_reserve builds them)", who);
            return -1;
        }
        return tcsc::kWideCW;
    }
    if (f == tcsc::kCW || !p->ent_w || p->order != TCSC_ORDER_FAST) return tcsc::kCW;
    if (slices != 1) return tcsc::kCW;
    return wide_pays(M, p->cols, p->num_cus) ? tcsc::kWideCW : tcsc::kCW;
}

}  // namespace

// The one place a call is routed (tcsc_plan.h).  The launch (sgemm_ws), the
// queries (tcsc_gpu_launch_info*, _geometry, _combine), the workspace sizes
// (tcsc_gpu_plan_workspace, tcsc_gpu_plan_reserve) and the host API's bands all
// read the value this returns; the cost models are asked here and nowhere else.
Route tcsc::route_call(const tcsc_gpu_plan* p, int M, int dt, size_t ws_avail, const RoutePins& pin, const char* who) {
    const XType& d = kXTypes[dt];
    const int K = p->rows, N = p->cols;
    Route r;
    r.path = pin.path != TCSC_PATH_AUTO ? pin.path : launch_path(p, M, dt);
    r.rows = std::min(M, kMaxLaunchRows);
    if (p->packed) {
        // The 2-bit image is the plan's only format: k_decode8 up to 16 rows (k_decode8r up to the plan's
        // decode_rows setting, §27), k_gemm8w2 above, whatever the cost models, $TCSC_PATH or $TCSC_DECODE say.  More than kMaxLaunchRows rows run in pieces of that
        // many on one workspace; every piece computes the same bits on either kernel and any K split.
        if (pin.path == TCSC_PATH_AUTO) r.path = use_decode(p, M, dt) ? TCSC_PATH_DECODE : TCSC_PATH_MFMA;
        if (r.path != TCSC_PATH_MFMA || !has_mfma(p, r.rows, dt)) return r;  // no workspace, or nothing to run
        r.slices = d.slices(r.rows, N, K);
        r.ws_bytes = mfma_ws(dt, r.rows, K, N).bytes;
        return r;
    }
    if (r.path == TCSC_PATH_MFMA) {  // [packed X][row flags][the GEMM's split-K slabs]: mfma_ws
        if (!has_mfma(p, M, dt)) return r;
        r.slices = d.slices(M, N, K);
        r.ws_bytes = mfma_ws(dt, M, K, N).bytes;
        return r;
    }
    if (r.path == TCSC_PATH_DECODE) return r;  // one launch that reads X in place: no workspace, K split inside the workgroup
    if (r.path == TCSC_PATH_SMALL) {
        // only the fp32 call has a staged form (tcsc_gpu_prepare_x's copy of X): the narrow types read X in place
        if (has_small(p, M) && dt == kF32) r.ws_bytes = align256((size_t)M * K * sizeof(float));
        return r;
    }
    // The gather, the same for every type: [X^T: xt_bytes(rows, K)][split-K slabs, if any].  A call of more
    // than kMaxLaunchRows rows runs in pieces of that many on one workspace, each with one K slice unless
    // the caller pins a split, so that a ragged last piece sums its rows in the same order as the full ones.
    const size_t xtb = tcsc::xt_bytes(r.rows, K);
    const int force = pin.slices > 0 ? pin.slices : M > kMaxLaunchRows ? 1 : slices_override();
    int chosen = 1;  // the reference orders walk K in order: never split
    if (p->order != TCSC_ORDER_REFERENCE)
        chosen = tcsc::choose_slices(r.rows, N, K, p->n_pos + p->n_neg, p->n_groups, ws_avail > xtb ? ws_avail - xtb : 0,
                                     force);
    r.slices = tcsc::normalized_slices(K, chosen);
    r.ws_bytes = xtb + tcsc::workspace_bytes(r.rows, N, chosen);  // as choose_slices counted them
    r.geo = launch_geo(p, r.rows, r.slices, force, who);
    if (r.slices > 1) {
        const long long cb = (p->n_groups + tcsc::kWaves - 1) / tcsc::kWaves, rt = (r.rows + tcsc::kTM - 1) / tcsc::kTM;
        const bool words = pin.plan_ws && p->csync != nullptr;  // the tile words belong to the plan's workspace
        r.combine = tcsc::combine_mode(r.slices, cb * rt * r.slices, cb * rt, (long long)r.rows * N,
                                       words ? p->num_cus : 0, words, pin.vec && N % 4 == 0);
    }
    return r;
}

namespace {
// the epilogue of an int8 call, for the kernels' launchers
I8Epi i8_epi(const Call& c) {
    I8Epi e;
    e.rscale = c.xscale;
    e.B = c.B;
    e.y = c.y;
    e.ldy = c.ldy;
    e.prelu = is_prelu(c.variant);
    e.a = c.a;
    e.R = c.R;
    e.ldr = c.ldr;
    return e;
}

// The MFMA path: pack X into the type's GEMM operand in the workspace, run
// the GEMM against W's image (the bias and PReLU in its store), and where the
// type keeps row flags rewrite the flagged rows exactly.
//   fp32: k_split3 (X -> X3 + flags), k_gemm3, k_fixup; stage 1 is the split
//         only, stage 2 the GEMM + fixup on the staged X3 (fp32 alone has stages)
//   bf16: k_pack1 (X -> X1 + flags, k_split3's rule), the one-part k_gemm3 and k_fixup
//   int8: k_pack8 (X -> X8), k_gemm8 against the int8 image (+ k_reduce_i8 when
//         K is split) with the row scales, the output descriptor's column
//         scales and Y type (§21); no flags, no fixup
int sgemm_mfma(const tcsc_gpu_plan* p, const Call& c, float* ws, size_t ws_bytes, int stage) {
    const int dt = c.xtype, M = c.M, ldy = c.ldy;
    const XType& d = kXTypes[dt];
    const void* dX = c.X;
    const float* dB = c.B;
    float* dY = static_cast<float*>(c.y.Y);  // the fp32 and bf16 calls write floats (y.plain())
    const float a = c.a;
    const int K = p->rows, N = p->cols, ldx = d.ldx(K), ldw = d.ldw(K);
    const MfmaWs w = mfma_ws(dt, M, K, N);
    if (!ws || ws_bytes < w.bytes) {
        set_error("%s: workspace of %zu bytes < %zu needed for M=%d", d.sgemm, ws ? ws_bytes : (size_t)0, w.bytes, M);
        return TCSC_E_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(c.stream);
    char* base = reinterpret_cast<char*>(ws);
    uint16_t* xp = reinterpret_cast<uint16_t*>(base);
    int* flags = reinterpret_cast<int*>(base + w.flags_off);
    void* slabs = base + w.slabs_off;
    const size_t slab_bytes = ws_bytes - w.slabs_off;
    const bool prelu = is_prelu(c.variant);
    switch (dt) {
        case kF32:
            if (stage != 2) HIP_TRY(tcsc::mfma_split_x(static_cast<const float*>(dX), M, K, xp, ldx, flags, st));
            if (stage == 1) return TCSC_OK;
            HIP_TRY(tcsc::mfma_gemm3(xp, ldx, p->wt, ldw, K, M, N, dB, dY, ldy, prelu, a, static_cast<float*>(slabs),
                                     slab_bytes, flags, p->ccq, p->crq, st));
            break;
        case kBf16:
            HIP_TRY(tcsc::mfma_pack_x(static_cast<const uint16_t*>(dX), M, K, xp, ldx, flags, st));
            HIP_TRY(tcsc::mfma_gemm1(xp, ldx, p->wt, ldw, K, M, N, dB, dY, ldy, prelu, a, static_cast<float*>(slabs),
                                     slab_bytes, flags, p->ccq, p->crq, st));
            break;
        case kI8: {
            HIP_TRY(tcsc::mfma8_pack_x(static_cast<const int8_t*>(dX), M, K, reinterpret_cast<int8_t*>(base), ldx, st));
            const I8Epi e = i8_epi(c);
            // B from the 2-bit image (k_gemm8w2): a packed plan has nothing else; an ordinary plan that has
            // both images takes it under $TCSC_W2GEMM=1 -- the same route, K split, workspace and bits
            if (p->packed || (p->w2 && w2gemm_knob()))
                HIP_TRY(tcsc::mfma8_gemm_w2(reinterpret_cast<const int8_t*>(base), p->w2, ldx, K, M, N, e,
                                            static_cast<int*>(slabs), slab_bytes, st));
            else
                HIP_TRY(tcsc::mfma8_gemm(reinterpret_cast<const int8_t*>(base), p->w8, ldx, K, M, N, e,
                                         static_cast<int*>(slabs), slab_bytes, st));
            break;
        }
    }
    // fast order: bias after the sum for every variant; a
    // split K rewrote the flagged rows in its reduce already
    if (d.flags && d.slices(M, N, K) <= 1) {
        const auto fixup = dt == kF32 ? tcsc::mfma_fixup : tcsc::mfma_fixup1;
        HIP_TRY(fixup(xp, M, K, ldx, p->ccq, p->crq, N, dB, dY, ldy, false, prelu, a, flags, st));
    }
    return TCSC_OK;
}

}  // namespace

// What the decode and MFMA routes of the int8 call can write and the others
// cannot: a bf16 Y, a column scale.  The gather and the small-M
// path finish in fp32 kernels shared with the fp32 call.
static const char* path_name(int path) {
    switch (path) {
        case TCSC_PATH_GATHER: return "gather";
        case TCSC_PATH_MFMA: return "MFMA";
        case TCSC_PATH_SMALL: return "small-M";
        case TCSC_PATH_DECODE: return "decode";
        default: return "unknown";
    }
}
static bool refuse_out(const char* who, int path, const YOut& y, int M) {
    if (y.plain() || path == TCSC_PATH_DECODE || path == TCSC_PATH_MFMA) return false;
    set_error("%s: %s%s%s needs the decode or the MFMA path, and M=%d routes to the %s path (%d), which writes an fp32 Y "
              "without column scales", who, y.ytype == kYBf16 ? "a bf16 Y" : "", y.ytype == kYBf16 && y.cscale ? " with " : "",
              y.cscale ? "a column scale" : "", M, path_name(path), path);
    return true;
}
// A residual is added in the epilogues of the same two routes.
static bool refuse_res(const char* who, int path, const void* R, int M) {
    if (!R || path == TCSC_PATH_DECODE || path == TCSC_PATH_MFMA) return false;
    set_error("%s: a residual needs the decode or the MFMA path, and M=%d routes to the %s path (%d), which has no "
              "residual add", who, M, path_name(path), path);
    return true;
}

// One call on the workspace ws: routed once (route_call, with what `pin`
// fixes and what the pointers allow), then launched as routed.
int tcsc::sgemm_ws(const tcsc_gpu_plan* p, const Call& c, float* ws, size_t ws_bytes, int stage, const RoutePins& pin,
                   Route* ran) {
    const int dt = c.xtype, M = c.M, ldy = c.ldy, variant = c.variant;
    const XType& d = kXTypes[dt];
    const char* who = c.who ? c.who : d.sgemm;
    const void* dX = c.X;
    const float *dScale = c.xscale, *dB = c.B;
    const YOut& y = c.y;
    float* dY = y.plain() ? static_cast<float*>(y.Y) : nullptr;  // the fp32 routes never see another Y
    const float a = c.a;
    void* stream = c.stream;
    if (dt != kI8 && !y.plain()) {
        set_error("%s: only the int8 call has a typed Y and column scales", who);
        return TCSC_E_ARG;
    }
    if (c.R && (dt != kI8 || stage != 0 || is_prelu(variant) || c.glu.up || c.group.count)) {
        set_error("%s: a residual goes with the plain int8 call alone (no PReLU, not gated, not grouped)", who);
        return TCSC_E_ARG;
    }
    if (dt != kF32 && stage != 0) {
        set_error("%s: no staged form", who);
        return TCSC_E_ARG;
    }
    if (!p || M < 0 || (stage != 1 && (ldy < p->cols || !valid_variant(variant)))) {
        set_error("%s: bad arguments (M=%d ldy=%d variant=%d)", who, M, ldy, variant);
        return TCSC_E_ARG;
    }
    if (p->packed && dt != kI8) {
        set_error("%s: a packed plan holds the 2-bit image only and runs tcsc_gpu_sgemm_i8 alone", who);
        return TCSC_E_ARG;
    }
    if (M == 0 || p->cols == 0) return TCSC_OK;
    if ((stage != 1 && (!y.Y || !dB)) || (stage != 2 && !dX && p->rows > 0)) {
        set_error("%s: NULL device pointer", who);
        return TCSC_E_ARG;
    }
    if (p->packed && M > kMaxLaunchRows) {  // pieces of at most kMaxLaunchRows rows on one workspace, each routed by its own rows
        for (int r0 = 0; r0 < M; r0 += kMaxLaunchRows) {
            const int rc = sgemm_ws(p, c.rows(r0, std::min(kMaxLaunchRows, M - r0), p->rows, d.elem), ws, ws_bytes, 0, pin,
                                    nullptr);
            if (rc != TCSC_OK) return rc;
        }
        if (ran) *ran = route_call(p, M, dt, ws ? ws_bytes : 0, pin);
        return TCSC_OK;
    }
    // the gather's arguments the route depends on: Y, B and the split-K slabs behind X^T
    const size_t xtb = tcsc::xt_bytes(std::min(M, kMaxLaunchRows), p->rows);
    tcsc::GemmArgs g;
    g.ncols = p->cols;
    g.B = dB;
    g.Y = dY;
    g.ldy = ldy;
    g.ws = (ws && ws_bytes > xtb) ? reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + xtb) : nullptr;
    g.ws_bytes = g.ws ? ws_bytes - xtb : 0;
    RoutePins pins = pin;
    pins.plan_ws = ws == p->ws;
    pins.vec = tcsc::stores16(g);
    // stage 1 only transposes: a geometry that cannot be had is the launch's error (stage 2)
    const Route r = route_call(p, M, dt, ws ? ws_bytes : 0, pins, stage != 1 ? who : nullptr);
    if (ran) *ran = r;
    if ((r.path == TCSC_PATH_MFMA && !has_mfma(p, M, dt)) || (r.path == TCSC_PATH_SMALL && !has_small(p, M)) ||
        (r.path == TCSC_PATH_DECODE && !has_decode(p, M, dt)) ||
        (p->packed && r.path != TCSC_PATH_MFMA && r.path != TCSC_PATH_DECODE)) {
        set_error("%s: the plan cannot run M=%d on the pinned path %d", who, M, r.path);
        return TCSC_E_ARG;
    }
    if (refuse_out(who, r.path, y, M) || refuse_res(who, r.path, c.R, M)) return TCSC_E_ARG;
    if (r.path == TCSC_PATH_DECODE) {
        HIP_TRY(tcsc::decode_gemm(tcsc::DecodeX{dX, kI8, nullptr, nullptr}, p->w2, p->rows, M, p->cols, i8_epi(c),
                                  p->num_cus, static_cast<hipStream_t>(stream)));
        return TCSC_OK;
    }
    if (r.path == TCSC_PATH_MFMA) return sgemm_mfma(p, c, ws, ws_bytes, stage);
    if (r.path == TCSC_PATH_SMALL) {
        // stage 1 stages X as is (the kernel reads X rows directly), stage 2 reads the staged copy
        hipStream_t st = static_cast<hipStream_t>(stream);
        const size_t xb = (size_t)M * p->rows * sizeof(float);
        if (stage != 0 && (!ws || ws_bytes < xb)) {
            set_error("tcsc_gpu_sgemm: workspace of %zu bytes < %zu needed for M=%d", ws ? ws_bytes : (size_t)0, xb,
                      M);
            return TCSC_E_ARG;
        }
        if (stage == 1) {
            HIP_TRY(hipMemcpyAsync(ws, dX, xb, hipMemcpyDeviceToDevice, st));
            return TCSC_OK;
        }
        HIP_TRY(tcsc::launch_small_m(stage == 2 ? ws : dX, dt, dScale, M, p->rows, p->ccq, p->crq, p->cols, dB, dY, ldy,
                                     false, is_prelu(variant), a, st));
        return TCSC_OK;
    }
    // At most kMaxLaunchRows rows per gather launch (tcsc_internal.h).  A
    // whole call (stage 0) runs as launches of that many rows (whole row
    // tiles) on the same workspace; the reference accepts any int M
    // (tcsc.c:69).  Every piece runs the whole call's route (one K slice
    // unless the caller pins a split), so a ragged last launch sums its rows
    // in the same order as the full ones (the workspace is sized for all of
    // M, which would otherwise let the cost model split K for a small tail:
    // ADVICE r3).
    if (M > kMaxLaunchRows) {
        if (stage != 0) {
            set_error("tcsc_gpu_sgemm: M=%d rows staged at once (at most %d; split the rows)", M, kMaxLaunchRows);
            return TCSC_E_ARG;
        }
        RoutePins piece = pin;
        piece.path = TCSC_PATH_GATHER;  // a short tail stays on the gather too
        piece.slices = r.slices;
        for (int r0 = 0; r0 < M; r0 += kMaxLaunchRows) {
            const int rc = sgemm_ws(p, c.rows(r0, std::min(kMaxLaunchRows, M - r0), p->rows, d.elem), ws, ws_bytes, 0,
                                    piece, nullptr);
            if (rc != TCSC_OK) return rc;
        }
        return TCSC_OK;
    }
    if (p->rows > 0 && (!ws || ws_bytes < xtb)) {
        set_error("%s: workspace of %zu bytes < %zu needed for M=%d", who, ws ? ws_bytes : (size_t)0, xtb, M);
        return TCSC_E_ARG;
    }
    g.X = dX;
    g.xtype = dt;
    g.Xscale = dScale;
    g.XT = p->rows > 0 ? ws : nullptr;
    g.M = M;
    g.K = p->rows;
    g.ent = p->ent;
    g.sptr = p->sptr;
    g.n_entries = p->n_entries;
    if (p->order == TCSC_ORDER_REFERENCE && p->chain_pos && p->chain_neg) {
        // basic / prelu_basic / sparseGEMM: one accumulator, +1 chain then
        // -1 chain; the optimized family: the two sums apart (k_stream ORDER 2)
        g.order = (variant == TCSC_VARIANT_BASIC || variant == TCSC_VARIANT_PRELU_BASIC ||
                   variant == TCSC_VARIANT_SPARSE_GEMM)
                      ? 1
                      : 2;
        g.ent = p->chain_pos->ent;
        g.sptr = p->chain_pos->sptr;
        g.n_entries = p->chain_pos->n_entries;
        g.ent2 = p->chain_neg->ent;
        g.sptr2 = p->chain_neg->sptr;
        g.n_entries2 = p->chain_neg->n_entries;
    }
    g.n_groups = p->n_groups;
    g.a = a;
    g.slices = r.slices;
    g.combine = r.combine;
    g.stage = stage;
    // the 22-column kernel where the rounds model (or $TCSC_GEO) says so: unsplit K, the wide streams
    if (stage != 1) {
        if (r.geo < 0) return TCSC_E_ARG;
        if (r.geo == tcsc::kWideCW) {
            g.geo = r.geo;
            g.ent = p->ent_w;
            g.sptr = p->sptr_w;
            g.wperm = p->wperm;
            g.n_entries = p->n_entries_w;
            g.n_groups = p->n_groups_w;
            g.slices = 1;
            g.combine = 0;
        }
    }
    // the plan's own workspace (device API) with its combine words, for the
    // in-launch split-K combine (the route says if it applies)
    if (pins.plan_ws && p->csync) {
        if (p->csync_dirty) {
            HIP_TRY(hipMemsetAsync(p->csync, 0, tcsc::kCombineBytes, static_cast<hipStream_t>(stream)));
            p->csync_dirty = false;
        }
        g.ccnt = p->csync;
        g.combine_giveup = combine_giveup_knob();
    }
    // The fast order (order 0) adds each column's nonzeros in ascending k and
    // the bias after the sum for every variant: the reference's own dense
    // oracle, dense.c:64-77 gemm_basic (y = 0; y += X*W; Y = y + B), bit for
    // bit when K is not split.  The reference order adds the
    // bias first for tcsc_sgemm_basic (tcsc.c:74-96) and sums the optimized
    // family's signs apart (order 2).
    g.bias_first = (g.order == 1 && variant == TCSC_VARIANT_BASIC);
    g.prelu = is_prelu(variant);
    hipError_t e = tcsc::launch_gemm(g, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        if (g.ccnt) p->csync_dirty = true;  // a partial launch may have left tile words set
        return hip_fail(e, "tcsc_gpu_sgemm launch");
    }
    return TCSC_OK;
}

// ===========================================================================
// Device-pointer API (include/tcsc_gpu.h)
// ===========================================================================
// tcsc_gpu_plan_create; allow_mfma false for the host API's exact mode
int tcsc::plan_create_impl(const tcsc_t* W, int col_begin, int col_end, int device, void* stream, bool allow_mfma,
                           tcsc_gpu_plan** out) {
    if (!W || !out || col_begin < 0 || col_end > W->cols || col_begin > col_end || W->rows < 0) {
        set_error("tcsc_gpu_plan_create: bad arguments");
        return TCSC_E_ARG;
    }
    *out = nullptr;
    const int nc = col_end - col_begin;
    std::vector<int> sorted_p, sorted_n;
    int rc = check_index_host(W->col_start_pos, W->row_index_pos, col_begin, col_end, W->rows, W->n_elem_pos, "pos",
                              sorted_p);
    if (rc == TCSC_OK)
        rc = check_index_host(W->col_start_neg, W->row_index_neg, col_begin, col_end, W->rows, W->n_elem_neg, "neg",
                              sorted_n);
    if (rc != TCSC_OK) return rc;
    DeviceGuard dg(device);
    if (!dg.ok()) {
        set_error("tcsc_gpu_plan_create: cannot select device %d", device);
        return TCSC_E_NODEV;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int p0 = W->col_start_pos[col_begin], p1 = W->col_start_pos[col_end];
    const int q0 = W->col_start_neg[col_begin], q1 = W->col_start_neg[col_end];
    const int* hrip = sorted_p.empty() ? W->row_index_pos + p0 : sorted_p.data();
    const int* hrin = sorted_n.empty() ? W->row_index_neg + q0 : sorted_n.data();
    // column slice, rebased to 0
    std::vector<int> csp(nc + 1), csn(nc + 1);
    for (int j = 0; j <= nc; ++j) {
        csp[j] = W->col_start_pos[col_begin + j] - p0;
        csn[j] = W->col_start_neg[col_begin + j] - q0;
    }
    DevBuf dcsp, dcsn, drip, drin;
    HIP_TRY(dcsp.alloc((nc + 1) * sizeof(int)));
    HIP_TRY(dcsn.alloc((nc + 1) * sizeof(int)));
    HIP_TRY(drip.alloc((size_t)(p1 - p0) * sizeof(int)));
    HIP_TRY(drin.alloc((size_t)(q1 - q0) * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(dcsp.p, csp.data(), (nc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dcsn.p, csn.data(), (nc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (p1 > p0)
        HIP_TRY(hipMemcpyAsync(drip.p, hrip, (size_t)(p1 - p0) * sizeof(int), hipMemcpyHostToDevice, st));
    if (q1 > q0)
        HIP_TRY(hipMemcpyAsync(drin.p, hrin, (size_t)(q1 - q0) * sizeof(int), hipMemcpyHostToDevice, st));
    rc = build_plan_ordered(W->rows, 0, nc, p1 - p0, q1 - q0, dcsp.as<int>(), dcsn.as<int>(), drip.as<int>(),
                            drin.as<int>(), device, st, current_order(), out, allow_mfma);
    if (rc == TCSC_OK) (*out)->col_begin = col_begin;
    return rc;
}

namespace {

// Entry points that need a format a packed plan lacks (fp32 or bf16 activations,
// the gather's queries, the staged pair, the transposed call): TCSC_E_ARG and a
// message that names the call, before any HIP call.
bool refuse_packed(const tcsc_gpu_plan* p, const char* who) {
    if (!p || !p->packed) return false;
    set_error("%s: not on a packed plan (it holds the 2-bit image only: tcsc_gpu_sgemm_i8, tcsc_gpu_launch_info_i8)", who);
    return true;
}

// What both packed constructors check before they touch the device.
int packed_args_ok(const char* who, int rows) {
    if (current_order() == TCSC_ORDER_REFERENCE) {
        set_error("%s: a packed plan has no reference-order form (TCSC_ORDER / tcsc_gpu_set_order ask for one)", who);
        return TCSC_E_ARG;
    }
    if (rows < 1 || rows >= tcsc::kDecodeMaxK) {
        set_error("%s: a packed plan needs 1 <= K < %d (K=%d)", who, tcsc::kDecodeMaxK, rows);
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}

// The packed plan of columns [col_begin, col_begin + ncols) of checked device
// TCSC arrays (absolute offsets): the 2-bit image by k_w2_from_tcsc and nothing
// else, so device_bytes is tcsc_gpu_w2_image_bytes(rows, ncols) exactly (the
// builder's flag word is freed before this returns).
int build_packed(const char* who, int rows, int col_begin, int ncols, long long n_pos, long long n_neg, const int* csp,
                 const int* csn, const int* rip, const int* rin, int device, hipStream_t st, tcsc_gpu_plan** out) {
    std::unique_ptr<tcsc_gpu_plan, PlanDeleter> plan(new tcsc_gpu_plan());
    plan->device = device;
    plan->rows = rows;
    plan->cols = ncols;
    plan->col_begin = col_begin;
    plan->n_pos = n_pos;
    plan->n_neg = n_neg;
    plan->packed = true;
    plan->mfma_min_M = tcsc::kDecodeMaxM + 1;
    HIP_TRY(hipDeviceGetAttribute(&plan->num_cus, hipDeviceAttributeMultiprocessorCount, device));
    if (ncols > 0) {
        const size_t bytes = tcsc::w2_image_bytes(rows, ncols);
        DevBuf bad;
        if (bad.alloc(sizeof(int)) != hipSuccess || hipMalloc(&plan->w2, bytes) != hipSuccess) {
            (void)hipGetLastError();
            plan->w2 = nullptr;
            set_error("%s: cannot allocate the 2-bit image (%zu bytes)", who, bytes);
            return TCSC_E_NOMEM;
        }
        plan->w2_bytes = bytes;
        int hbad = 0;
        HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int), st));
        HIP_TRY(tcsc::w2_from_tcsc(csp, csn, rip, rin, col_begin, ncols, rows, plan->w2, bad.as<int>(), st));
        HIP_TRY(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (hbad) {
            set_error("%s: W is not ternary: a position's summed weight is outside {-1, 0, +1} (a duplicated index)", who);
            return TCSC_E_ARG;
        }
    }
    *out = plan.release();
    return TCSC_OK;
}

// ---- packed plans and TCSC arrays from a saved image -----------
// What every entry point that takes an image refuses on the host, before any
// HIP call.
int image_args_ok(const char* who, const void* image, size_t bytes, int rows, int cols) {
    if (!image) {
        set_error("%s: NULL image", who);
        return TCSC_E_ARG;
    }
    if (rows < 1 || rows >= tcsc::kDecodeMaxK) {
        set_error("%s: an image needs 1 <= K < %d (rows=%d)", who, tcsc::kDecodeMaxK, rows);
        return TCSC_E_ARG;
    }
    if (cols < 1) {
        set_error("%s: cols must be at least 1 (cols=%d)", who, cols);
        return TCSC_E_ARG;
    }
    if (bytes != tcsc::w2_image_bytes(rows, cols)) {
        set_error("%s: bytes=%zu is not tcsc_gpu_w2_image_bytes(%d, %d) = %zu", who, bytes, rows, cols,
                  tcsc::w2_image_bytes(rows, cols));
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}

// k_w2_check on a device image: the counts, or TCSC_E_ARG naming the fault.
// Synchronises st.
int check_image(const char* who, const uint32_t* w2, int rows, int cols, long long* n_pos, long long* n_neg,
                hipStream_t st) {
    struct Acc {
        unsigned long long n[2];  // +1, -1
        int bad, pad;
    } h = {{0, 0}, 0, 0};
    DevBuf acc;
    HIP_TRY(acc.alloc(sizeof(Acc)));
    HIP_TRY(hipMemsetAsync(acc.p, 0, sizeof(Acc), st));
    Acc* d = acc.as<Acc>();
    HIP_TRY(tcsc::w2_check(w2, cols, rows, d->n, &d->bad, st));
    HIP_TRY(hipMemcpyAsync(&h, acc.p, sizeof(Acc), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int bad = h.bad;
    if (bad) {
        set_error("%s: invalid image: %s%s%s", who, bad & tcsc::kW2BadCode ? "a code 3 (no ternary weight)" : "",
                  bad == (tcsc::kW2BadCode | tcsc::kW2BadPad) ? "; " : "",
                  bad & tcsc::kW2BadPad ? "padding (k >= rows or column >= cols) holds a code other than 1" : "");
        return TCSC_E_ARG;
    }
    *n_pos = (long long)h.n[0];
    *n_neg = (long long)h.n[1];
    return TCSC_OK;
}

// tcsc_gpu_plan_create_packed_image / _device: the plan's own copy of the image
// (`kind` says where `image` lives), validated and counted by k_w2_check.
int packed_from_image(const char* who, const void* image, hipMemcpyKind kind, size_t bytes, int rows, int cols,
                      int col_begin, int device, void* stream, tcsc_gpu_plan** out) {
    if (!out) {
        set_error("%s: NULL out", who);
        return TCSC_E_ARG;
    }
    *out = nullptr;
    int rc = image_args_ok(who, image, bytes, rows, cols);
    if (rc == TCSC_OK) rc = packed_args_ok(who, rows);
    if (rc != TCSC_OK) return rc;
    if (col_begin < 0) {
        set_error("%s: col_begin must not be negative (col_begin=%d)", who, col_begin);
        return TCSC_E_ARG;
    }
    DeviceGuard dg(device);
    if (!dg.ok()) {
        set_error("%s: cannot select device %d", who, device);
        return TCSC_E_NODEV;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::unique_ptr<tcsc_gpu_plan, PlanDeleter> plan(new tcsc_gpu_plan());  // the fields build_packed sets
    plan->device = device;
    plan->rows = rows;
    plan->cols = cols;
    plan->col_begin = col_begin;
    plan->packed = true;
    plan->mfma_min_M = tcsc::kDecodeMaxM + 1;
    HIP_TRY(hipDeviceGetAttribute(&plan->num_cus, hipDeviceAttributeMultiprocessorCount, device));
    if (hipMalloc(&plan->w2, bytes) != hipSuccess) {
        (void)hipGetLastError();
        plan->w2 = nullptr;
        set_error("%s: cannot allocate the 2-bit image (%zu bytes)", who, bytes);
        return TCSC_E_NOMEM;
    }
    plan->w2_bytes = bytes;
    HIP_TRY(hipMemcpyAsync(plan->w2, image, bytes, kind, st));
    rc = check_image(who, plan->w2, rows, cols, &plan->n_pos, &plan->n_neg, st);
    if (rc != TCSC_OK) return rc;  // the plan and its copy are freed here
    *out = plan.release();
    return TCSC_OK;
}

}  // namespace

extern "C" {

int tcsc_gpu_device_count(void) { return device_count_raw(); }

const char* tcsc_gpu_last_error(void) { return g_last_error.c_str(); }

int tcsc_gpu_plan_create(const tcsc_t* W, int col_begin, int col_end, int device, void* stream,
                         tcsc_gpu_plan** out) {
    return tcsc::plan_create_impl(W, col_begin, col_end, device, stream, true, out);
}

int tcsc_gpu_plan_create_device(int rows, int cols, const int* d_csp, const int* d_csn, const int* d_rip,
                                const int* d_rin, int col_begin, int col_end, int device, void* stream,
                                tcsc_gpu_plan** out) {
    if (!out || !d_csp || !d_csn || col_begin < 0 || col_end > cols || col_begin > col_end || rows < 0) {
        set_error("tcsc_gpu_plan_create_device: bad arguments");
        return TCSC_E_ARG;
    }
    *out = nullptr;
    DeviceGuard dg(device);
    if (!dg.ok()) {
        set_error("tcsc_gpu_plan_create_device: cannot select device %d", device);
        return TCSC_E_NODEV;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    int ends[4];
    HIP_TRY(hipMemcpyAsync(&ends[0], d_csp + col_begin, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[1], d_csp + col_end, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[2], d_csn + col_begin, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[3], d_csn + col_end, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the same preconditions as tcsc_gpu_plan_create's host check, on the
    // device: a bad range is an error, columns out of order are sorted
    const int nc = col_end - col_begin;
    DevBuf flag;
    HIP_TRY(flag.alloc(sizeof(int)));
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    HIP_TRY(tcsc::check_index_device(d_csp, d_rip, col_begin, nc, rows, ends[1], flag.as<int>(), st));
    HIP_TRY(tcsc::check_index_device(d_csn, d_rin, col_begin, nc, rows, ends[3], flag.as<int>(), st));
    int hflag = 0;
    HIP_TRY(hipMemcpyAsync(&hflag, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hflag & 1) {
        set_error("tcsc_gpu_plan_create_device: a col_start range or a row index outside [0, %d)", rows);
        return TCSC_E_ARG;
    }
    if (!(hflag & 2))
        return build_plan_ordered(rows, col_begin, nc, ends[1] - ends[0], ends[3] - ends[2], d_csp, d_csn, d_rip,
                                  d_rin, device, st, current_order(), out);
    // columns out of order: rebased offsets and per-column sorted copies
    const int np = ends[1] - ends[0], nn = ends[3] - ends[2];
    DevBuf ocp, ocn, srp, srn, tmp;
    HIP_TRY(ocp.alloc((size_t)(nc + 1) * sizeof(int)));
    HIP_TRY(ocn.alloc((size_t)(nc + 1) * sizeof(int)));
    HIP_TRY(srp.alloc((size_t)np * sizeof(int)));
    HIP_TRY(srn.alloc((size_t)nn * sizeof(int)));
    size_t tb1 = 0, tb2 = 0;
    HIP_TRY(tcsc::sort_columns_tmp_bytes(np, nc, &tb1));
    HIP_TRY(tcsc::sort_columns_tmp_bytes(nn, nc, &tb2));
    const size_t tb = tb1 > tb2 ? tb1 : tb2;
    HIP_TRY(tmp.alloc(tb));
    HIP_TRY(tcsc::rebase_offsets(d_csp, col_begin, nc, ocp.as<int>(), st));
    HIP_TRY(tcsc::rebase_offsets(d_csn, col_begin, nc, ocn.as<int>(), st));
    HIP_TRY(tcsc::sort_columns(d_rip + ends[0], srp.as<int>(), np, nc, ocp.as<int>(), tmp.p, tb, st));
    HIP_TRY(tcsc::sort_columns(d_rin + ends[2], srn.as<int>(), nn, nc, ocn.as<int>(), tmp.p, tb, st));
    const int rc = build_plan_ordered(rows, 0, nc, np, nn, ocp.as<int>(), ocn.as<int>(), srp.as<int>(),
                                      srn.as<int>(), device, st, current_order(), out);
    if (rc == TCSC_OK) (*out)->col_begin = col_begin;
    return rc;
}

int tcsc_gpu_plan_create_packed(const tcsc_t* W, int col_begin, int col_end, int device, void* stream,
                                tcsc_gpu_plan** out) {
    const char* who = "tcsc_gpu_plan_create_packed";
    if (!W || !out || col_begin < 0 || col_end > W->cols || col_begin > col_end) {
        set_error("%s: bad arguments", who);
        return TCSC_E_ARG;
    }
    *out = nullptr;
    int rc = packed_args_ok(who, W->rows);
    if (rc != TCSC_OK) return rc;
    // ranges and rows as tcsc_gpu_plan_create checks them; the order inside a column does not reach the image
    std::vector<int> unused;
    rc = check_index_host(W->col_start_pos, W->row_index_pos, col_begin, col_end, W->rows, W->n_elem_pos, "pos", unused);
    if (rc == TCSC_OK)
        rc = check_index_host(W->col_start_neg, W->row_index_neg, col_begin, col_end, W->rows, W->n_elem_neg, "neg",
                              unused);
    if (rc != TCSC_OK) return rc;
    DeviceGuard dg(device);
    if (!dg.ok()) {
        set_error("%s: cannot select device %d", who, device);
        return TCSC_E_NODEV;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nc = col_end - col_begin;
    const int p0 = W->col_start_pos[col_begin], p1 = W->col_start_pos[col_end];
    const int q0 = W->col_start_neg[col_begin], q1 = W->col_start_neg[col_end];
    std::vector<int> csp(nc + 1), csn(nc + 1);  // the column slice, rebased to 0
    for (int j = 0; j <= nc; ++j) {
        csp[j] = W->col_start_pos[col_begin + j] - p0;
        csn[j] = W->col_start_neg[col_begin + j] - q0;
    }
    DevBuf dcsp, dcsn, drip, drin;  // upload scratch, freed on return
    HIP_TRY(dcsp.alloc((nc + 1) * sizeof(int)));
    HIP_TRY(dcsn.alloc((nc + 1) * sizeof(int)));
    HIP_TRY(drip.alloc((size_t)(p1 - p0) * sizeof(int)));
    HIP_TRY(drin.alloc((size_t)(q1 - q0) * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(dcsp.p, csp.data(), (nc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dcsn.p, csn.data(), (nc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (p1 > p0)
        HIP_TRY(hipMemcpyAsync(drip.p, W->row_index_pos + p0, (size_t)(p1 - p0) * sizeof(int), hipMemcpyHostToDevice, st));
    if (q1 > q0)
        HIP_TRY(hipMemcpyAsync(drin.p, W->row_index_neg + q0, (size_t)(q1 - q0) * sizeof(int), hipMemcpyHostToDevice, st));
    rc = build_packed(who, W->rows, 0, nc, p1 - p0, q1 - q0, dcsp.as<int>(), dcsn.as<int>(), drip.as<int>(),
                      drin.as<int>(), device, st, out);
    if (rc == TCSC_OK) (*out)->col_begin = col_begin;
    return rc;
}

int tcsc_gpu_plan_create_packed_device(int rows, int cols, const int* d_csp, const int* d_csn, const int* d_rip,
                                       const int* d_rin, int col_begin, int col_end, int device, void* stream,
                                       tcsc_gpu_plan** out) {
    const char* who = "tcsc_gpu_plan_create_packed_device";
    if (!out || !d_csp || !d_csn || col_begin < 0 || col_end > cols || col_begin > col_end) {
        set_error("%s: bad arguments", who);
        return TCSC_E_ARG;
    }
    *out = nullptr;
    const int rc = packed_args_ok(who, rows);
    if (rc != TCSC_OK) return rc;
    DeviceGuard dg(device);
    if (!dg.ok()) {
        set_error("%s: cannot select device %d", who, device);
        return TCSC_E_NODEV;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    int ends[4];
    HIP_TRY(hipMemcpyAsync(&ends[0], d_csp + col_begin, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[1], d_csp + col_end, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[2], d_csn + col_begin, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[3], d_csn + col_end, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // tcsc_gpu_plan_create_device's check: a bad range or row is an error; columns out of order are fine here
    const int nc = col_end - col_begin;
    DevBuf flag;
    HIP_TRY(flag.alloc(sizeof(int)));
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    HIP_TRY(tcsc::check_index_device(d_csp, d_rip, col_begin, nc, rows, ends[1], flag.as<int>(), st));
    HIP_TRY(tcsc::check_index_device(d_csn, d_rin, col_begin, nc, rows, ends[3], flag.as<int>(), st));
    int hflag = 0;
    HIP_TRY(hipMemcpyAsync(&hflag, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hflag & 1) {
        set_error("%s: a col_start range or a row index outside [0, %d)", who, rows);
        return TCSC_E_ARG;
    }
    return build_packed(who, rows, col_begin, nc, ends[1] - ends[0], ends[3] - ends[2], d_csp, d_csn, d_rip, d_rin,
                        device, st, out);
}

int tcsc_gpu_plan_is_packed(const tcsc_gpu_plan* p) {
    if (!p) {
        set_error("tcsc_gpu_plan_is_packed: NULL plan");
        return 0;
    }
    return p->packed ? 1 : 0;
}

int tcsc_gpu_plan_copy_w2(const tcsc_gpu_plan* p, void* d_dst, size_t bytes, void* stream) {
    if (!p) {
        set_error("tcsc_gpu_plan_copy_w2: NULL plan");
        return TCSC_E_ARG;
    }
    if (!p->w2 || bytes != p->w2_bytes || !d_dst) {
        set_error("tcsc_gpu_plan_copy_w2: %s", !p->w2 ? "the plan has no 2-bit image"
                                                      : !d_dst ? "NULL destination" : "bytes is not the image's size");
        return TCSC_E_ARG;
    }
    DeviceGuard dg(p->device);
    HIP_TRY(hipMemcpyAsync(d_dst, p->w2, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return TCSC_OK;
}

int tcsc_gpu_plan_create_packed_image(const void* image, size_t bytes, int rows, int cols, int col_begin, int device,
                                      void* stream, tcsc_gpu_plan** out) {
    return packed_from_image("tcsc_gpu_plan_create_packed_image", image, hipMemcpyHostToDevice, bytes, rows, cols,
                             col_begin, device, stream, out);
}

int tcsc_gpu_plan_create_packed_image_device(const void* d_image, size_t bytes, int rows, int cols, int col_begin,
                                             int device, void* stream, tcsc_gpu_plan** out) {
    return packed_from_image("tcsc_gpu_plan_create_packed_image_device", d_image, hipMemcpyDeviceToDevice, bytes, rows,
                             cols, col_begin, device, stream, out);
}

int tcsc_gpu_w2_to_tcsc(const void* d_image, size_t bytes, int rows, int cols, int* d_csp, int* d_csn, int* d_rip,
                        int* d_rin, int* n_pos, int* n_neg, void* stream) {
    const char* who = "tcsc_gpu_w2_to_tcsc";
    if (!d_csp || !d_csn || !n_pos || !n_neg) {
        set_error("%s: NULL col_start or count pointer", who);
        return TCSC_E_ARG;
    }
    int rc = image_args_ok(who, d_image, bytes, rows, cols);
    if (rc != TCSC_OK) return rc;
    if (!tcsc::w2_unpack_fits(cols, rows)) {
        set_error("%s: %d columns x %d k blocks do not fit 32-bit counters", who, cols, tcsc::w2_kblocks(rows));
        return TCSC_E_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t* w2 = static_cast<const uint32_t*>(d_image);
    long long np = 0, nn = 0;
    rc = check_image(who, w2, rows, cols, &np, &nn, st);
    if (rc != TCSC_OK) return rc;
    if (np > 0x7fffffffLL || nn > 0x7fffffffLL) {
        set_error("%s: %lld +1 and %lld -1 entries: tcsc_t offsets are int (each sign below 2^31)", who, np, nn);
        return TCSC_E_ARG;
    }
    // per (column, k block) counts, their exclusive scans, col_start out of those
    const size_t n = (size_t)cols * tcsc::w2_kblocks(rows) + 1;
    size_t tb = 0;
    HIP_TRY(tcsc::plan_scan_tmp_bytes((long long)n, &tb));
    const size_t arr = align256(n * sizeof(int));
    DevBuf scratch;  // one allocation: [scan scratch][cntp][cntn][offp][offn]
    HIP_TRY(scratch.alloc(align256(tb) + 4 * arr));
    char* base = scratch.as<char>() + align256(tb);
    int *cntp = reinterpret_cast<int*>(base), *cntn = reinterpret_cast<int*>(base + arr);
    int *offp = reinterpret_cast<int*>(base + 2 * arr), *offn = reinterpret_cast<int*>(base + 3 * arr);
    HIP_TRY(hipMemsetAsync(cntp + (n - 1), 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(cntn + (n - 1), 0, sizeof(int), st));
    HIP_TRY(tcsc::w2_unpack_counts(w2, cols, rows, cntp, cntn, st));
    HIP_TRY(tcsc::exclusive_scan_i32(cntp, offp, (int)n, scratch.p, tb, st));
    HIP_TRY(tcsc::exclusive_scan_i32(cntn, offn, (int)n, scratch.p, tb, st));
    HIP_TRY(tcsc::w2_unpack_col_start(offp, offn, cols, rows, d_csp, d_csn, st));
    if (d_rip && d_rin) HIP_TRY(tcsc::w2_unpack_fill(w2, cols, rows, offp, offn, d_rip, d_rin, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_pos = (int)np;
    *n_neg = (int)nn;
    return TCSC_OK;
}

int tcsc_gpu_plan_get_info(const tcsc_gpu_plan* p, tcsc_gpu_plan_info* info) {
    if (!p || !info) {
        set_error("tcsc_gpu_plan_get_info: NULL");
        return TCSC_E_ARG;
    }
    info->device = p->device;
    info->rows = p->rows;
    info->cols = p->cols;
    info->col_begin = p->col_begin;
    info->nnz = p->n_pos + p->n_neg;
    info->n_pos = p->n_pos;
    info->n_neg = p->n_neg;
    info->chunk_k = tcsc::kTK;
    info->n_chunks = p->n_chunks;
    info->device_bytes = p->bytes + p->ws_bytes + p->mfma_bytes + p->i8_bytes + p->w2_bytes + p->csc_bytes + p->tbias_bytes + p->wide_bytes +
                         (p->chain_pos ? p->chain_pos->bytes : 0) + (p->chain_neg ? p->chain_neg->bytes : 0);
    info->order = p->order;
    info->mfma_min_M = (p->wt || p->packed) ? p->mfma_min_M : 0;  // packed: k_gemm8w2 from 17 rows
    return TCSC_OK;
}

void tcsc_gpu_set_order(int order) {
    std::lock_guard<std::mutex> lk(g_order_mu);
    g_order = order == TCSC_ORDER_REFERENCE ? TCSC_ORDER_REFERENCE : TCSC_ORDER_FAST;
}

int tcsc_gpu_get_order(void) { return current_order(); }

void tcsc_gpu_plan_destroy(tcsc_gpu_plan* p) {
    if (!p) return;
    DeviceGuard dg(p->device);
    if (p->ent) (void)hipFree(p->ent);
    if (p->sptr) (void)hipFree(p->sptr);
    if (p->ws) (void)hipFree(p->ws);
    if (p->csync) (void)hipFree(p->csync);
    if (p->tbias) (void)hipFree(p->tbias);
    if (p->ent_w) (void)hipFree(p->ent_w);
    if (p->sptr_w) (void)hipFree(p->sptr_w);
    if (p->wperm) (void)hipFree(p->wperm);
    free_mfma(p);
    free_csc(p);
    tcsc_gpu_plan_destroy(p->chain_pos);
    tcsc_gpu_plan_destroy(p->chain_neg);
    delete p;
}

int tcsc_gpu_plan_reserve(tcsc_gpu_plan* p, int max_M) {
    if (!p || max_M < 0) {
        set_error("tcsc_gpu_plan_reserve: bad arguments");
        return TCSC_E_ARG;
    }
    const size_t want = reserve_bytes(p, max_M);
    if (!p->csync && p->rows > 0 && p->order == TCSC_ORDER_FAST && !p->packed) {  // the gather's tile words
        DeviceGuard dg(p->device);
        HIP_TRY(hipMalloc(&p->csync, tcsc::kCombineBytes));
        HIP_TRY(hipMemset(p->csync, 0, tcsc::kCombineBytes));
        HIP_TRY(hipDeviceSynchronize());
        if (!p->num_cus) HIP_TRY(hipDeviceGetAttribute(&p->num_cus, hipDeviceAttributeMultiprocessorCount, p->device));
    }
    // the wide streams, where a launch of some M <= max_M takes them: built
    // here so that no launch after this call allocates or synchronises
    if (!p->ent_w && wide_wanted(p, max_M)) {
        const int rc = build_wide(p);
        if (rc != TCSC_OK) return rc;
    }
    if (want <= p->ws_bytes) return TCSC_OK;
    DeviceGuard dg(p->device);
    if (p->ws) {
        HIP_TRY(hipDeviceSynchronize());  // a queued launch may still use it
        (void)hipFree(p->ws);
    }
    p->ws = nullptr;
    p->ws_bytes = 0;
    p->staged_M = -1;
    HIP_TRY(hipMalloc(&p->ws, want));
    p->ws_bytes = want;
    return TCSC_OK;
}

int tcsc_gpu_plan_workspace(const tcsc_gpu_plan* p, int M, int path, size_t* need, size_t* reserved) {
    if (!p || M < 0 || (path != TCSC_PATH_AUTO && path != TCSC_PATH_GATHER && path != TCSC_PATH_MFMA &&
                        path != TCSC_PATH_SMALL && path != TCSC_PATH_DECODE)) {
        set_error("tcsc_gpu_plan_workspace: bad arguments (M=%d path=%d)", M, path);
        return TCSC_E_ARG;
    }
    if (need) *need = path_ws_bytes(p, M, path);
    if (reserved) *reserved = p->ws_bytes;
    return TCSC_OK;
}

// What the queries report: the route of a tcsc_gpu_sgemm* of M rows on the
// plan's own workspace as reserved now, with aligned pointers and ldy % 4 == 0.
static Route plan_route(const tcsc_gpu_plan* p, int M, int dt, const char* who = nullptr) {
    return route_call(p, M, dt, p->ws_bytes, RoutePins(), who);
}

static int launch_info_impl(const char* who, const tcsc_gpu_plan* p, int M, int* path, int* slices, int dt) {
    if (!p || M < 0 || !path || !slices) {
        set_error("%s: bad arguments", who);
        return TCSC_E_ARG;
    }
    if (dt != kI8 && refuse_packed(p, who)) return TCSC_E_ARG;
    const Route r = plan_route(p, M, dt);
    *path = r.path;
    *slices = r.slices;
    return TCSC_OK;
}

int tcsc_gpu_launch_info(const tcsc_gpu_plan* p, int M, int* path, int* slices) {
    return launch_info_impl("tcsc_gpu_launch_info", p, M, path, slices, kF32);
}

int tcsc_gpu_launch_info_bf16(const tcsc_gpu_plan* p, int M, int* path, int* slices) {
    return launch_info_impl("tcsc_gpu_launch_info_bf16", p, M, path, slices, kBf16);
}

int tcsc_gpu_launch_info_i8(const tcsc_gpu_plan* p, int M, int* path, int* slices) {
    return launch_info_impl("tcsc_gpu_launch_info_i8", p, M, path, slices, kI8);
}

int tcsc_gpu_wide_pays(int M, int ncols, int num_cus) { return wide_pays(M, ncols, num_cus) ? 1 : 0; }

int tcsc_gpu_plan_wide_stats(const tcsc_gpu_plan* p, long long stats[4], unsigned short* map, size_t map_entries) {
    if (!p || (!stats && !map)) {
        set_error("tcsc_gpu_plan_wide_stats: bad arguments");
        return TCSC_E_ARG;
    }
    if (!p->ent_w || !p->wperm) {
        set_error("tcsc_gpu_plan_wide_stats: the plan has no wide streams (tcsc_gpu_plan_reserve builds them)");
        return TCSC_E_ARG;
    }
    if (stats)
        for (int i = 0; i < 4; ++i) stats[i] = p->wide_stats[i];
    if (map) {
        const size_t nmap = (size_t)tcsc::wide_blocks_for(p->cols) * tcsc::kWideWgCols;
        if (map_entries != nmap) {
            set_error("tcsc_gpu_plan_wide_stats: the map has %zu entries, not %zu", nmap, map_entries);
            return TCSC_E_ARG;
        }
        DeviceGuard dg(p->device);
        HIP_TRY(hipMemcpy(map, p->wperm, nmap * sizeof(unsigned short), hipMemcpyDeviceToHost));
    }
    return TCSC_OK;
}

int tcsc_gpu_launch_geometry(const tcsc_gpu_plan* p, int M, int* cols_per_wave) {
    if (!p || M < 0 || !cols_per_wave) {
        set_error("tcsc_gpu_launch_geometry: bad arguments");
        return TCSC_E_ARG;
    }
    if (refuse_packed(p, "tcsc_gpu_launch_geometry")) return TCSC_E_ARG;
    *cols_per_wave = 0;  // not a gather launch
    const Route r = plan_route(p, M, kF32, "tcsc_gpu_launch_geometry");
    if (r.path != TCSC_PATH_GATHER) return TCSC_OK;
    if (r.geo < 0) return TCSC_E_ARG;
    *cols_per_wave = r.geo;
    return TCSC_OK;
}

int tcsc_gpu_launch_combine(const tcsc_gpu_plan* p, int M, int* in_launch) {
    if (!p || M < 0 || !in_launch) {
        set_error("tcsc_gpu_launch_combine: bad arguments");
        return TCSC_E_ARG;
    }
    if (refuse_packed(p, "tcsc_gpu_launch_combine")) return TCSC_E_ARG;
    *in_launch = plan_route(p, M, kF32).combine;  // 0 off the gather path and where K is not split
    return TCSC_OK;
}

// tcsc_gpu_sgemm{,_bf16,_i8}: grow the workspace on first use at a larger M
// (tcsc_gpu_plan_reserve up front keeps the call allocation-free and
// graph-capturable: its size covers every launch of every type, mfma_ws),
// then run on it.
// A route that cannot write the typed Y or the column scales the call asks for
// (the int8 call's _out form) is refused here, ahead of the workspace and of
// any launch.
static int sgemm_entry(const tcsc_gpu_plan* p, const Call& c) {
    const int dt = c.xtype, M = c.M;
    if (dt != kI8 && refuse_packed(p, kXTypes[dt].sgemm)) return TCSC_E_ARG;
    if ((!c.y.plain() || c.R) && p && M > 0 && p->cols > 0) {
        const char* who = c.who ? c.who : kXTypes[dt].sgemm;
        const int path = route_call(p, M, dt, p->ws_bytes, RoutePins()).path;
        if (refuse_out(who, path, c.y, M) || refuse_res(who, path, c.R, M)) return TCSC_E_ARG;
    }
    if (p && M > 0 && p->cols > 0 && p->ws_bytes < wanted_workspace(p, M, dt)) {
        const int rc = tcsc_gpu_plan_reserve(const_cast<tcsc_gpu_plan*>(p), M);
        if (rc != TCSC_OK) return rc;
    }
    if (p) const_cast<tcsc_gpu_plan*>(p)->staged_M = -1;  // this call's X^T or packed X replaces any staged one
    return sgemm_ws(p, c, p ? p->ws : nullptr, p ? p->ws_bytes : 0, 0, RoutePins(), nullptr);
}

static YOut y_out(void* dY, int ytype, const float* dColScale) {
    return YOut{dY, ytype == TCSC_Y_BF16 ? kYBf16 : kYF32, dColScale};
}

int tcsc_gpu_sgemm(const tcsc_gpu_plan* p, const float* dX, const float* dB, float* dY, int M, int ldy,
                   int variant, float a, void* stream) {
    return sgemm_entry(p, make_call(dX, kF32, nullptr, dB, YOut{dY, kYF32, nullptr}, M, ldy, variant, a, stream));
}

int tcsc_gpu_sgemm_bf16(const tcsc_gpu_plan* p, const void* dX_bf16, const float* dB, float* dY, int M, int ldy,
                        int variant, float a, void* stream) {
    return sgemm_entry(p, make_call(dX_bf16, kBf16, nullptr, dB, YOut{dY, kYF32, nullptr}, M, ldy, variant, a, stream));
}

int tcsc_gpu_plan_enable_i8(tcsc_gpu_plan* p, void* stream) {
    if (!p) {
        set_error("tcsc_gpu_plan_enable_i8: NULL plan");
        return TCSC_E_ARG;
    }
    // only beside the bf16 image of a fast-order plan; anything else stays as it was
    if (p->w8 || !p->wt || p->order == TCSC_ORDER_REFERENCE || p->rows <= 0 || p->cols <= 0) return TCSC_OK;
    DeviceGuard dg(p->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ld8 = tcsc::mfma8_ldw(p->rows);
    const size_t bytes = (size_t)p->cols * ld8;
    DevBuf bad;
    if (bad.alloc(sizeof(int)) != hipSuccess || hipMalloc(&p->w8, bytes) != hipSuccess) {
        (void)hipGetLastError();
        p->w8 = nullptr;
        set_error("tcsc_gpu_plan_enable_i8: cannot allocate the int8 image (%zu bytes)", bytes);
        return TCSC_E_NOMEM;
    }
    p->i8_bytes = bytes;
    int hbad = 0, rc = TCSC_OK;
    hipError_t e = hipMemsetAsync(bad.p, 0, sizeof(int), st);
    if (e == hipSuccess)
        e = tcsc::mfma8_build_w8(p->wt, p->cols, p->rows, tcsc::mfma_ldw(p->rows), p->w8, ld8, bad.as<int>(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = hip_fail(e, "tcsc_gpu_plan_enable_i8");
    // a weight beyond int8, or a column whose sum of |w| could carry an i32 sum past 2^31: no image
    if (rc != TCSC_OK || hbad) free_i8(p);
    return rc;
}

int tcsc_gpu_plan_set_decode_rows(tcsc_gpu_plan* p, int rows) {
    if (!p) {
        set_error("tcsc_gpu_plan_set_decode_rows: NULL plan");
        return TCSC_E_ARG;
    }
    if (rows != TCSC_DECODE_ROWS_AUTO && (rows < tcsc::kDecodeMaxM || rows > tcsc::kDecodeRowsMax)) {
        set_error("tcsc_gpu_plan_set_decode_rows: rows=%d is neither %d .. %d nor TCSC_DECODE_ROWS_AUTO", rows,
                  tcsc::kDecodeMaxM, tcsc::kDecodeRowsMax);
        return TCSC_E_ARG;
    }
    if (!p->w2) {
        set_error("tcsc_gpu_plan_set_decode_rows: the plan has no 2-bit image (tcsc_gpu_plan_enable_w2, or a packed plan)");
        return TCSC_E_ARG;
    }
    p->decode_rows = rows;  // read per call by route_call: nothing is allocated, freed or synchronised
    return TCSC_OK;
}

int tcsc_gpu_plan_decode_rows(const tcsc_gpu_plan* p) {
    if (!p) {
        set_error("tcsc_gpu_plan_decode_rows: NULL plan");
        return TCSC_E_ARG;
    }
    return p->decode_rows;
}

int tcsc_gpu_decode_rows_pays(int M, int K, int N, int num_cus) { return decode_rows_pays(M, K, N, num_cus) ? 1 : 0; }

int tcsc_gpu_launch_info_decode(const tcsc_gpu_plan* p, int M, int* row_tiles, int* col_tiles, long long* workgroups) {
    if (!p || !row_tiles || !col_tiles || !workgroups) {
        set_error("tcsc_gpu_launch_info_decode: bad arguments");
        return TCSC_E_ARG;
    }
    if (!p->w2 || M < 1 || M > tcsc::kDecodeRowsMax) {
        set_error("tcsc_gpu_launch_info_decode: no decode launch of M=%d rows (1 .. %d on a plan with the 2-bit image)", M,
                  tcsc::kDecodeRowsMax);
        return TCSC_E_ARG;
    }
    const int rt = tcsc::decode_row_tiles(M);
    const int t = rt > 1 ? tcsc::decode_rows_tiles_per_wg(M, p->cols, p->num_cus)
                         : tcsc::decode_tiles_per_wg(M, p->cols, p->num_cus);
    *row_tiles = rt;
    *col_tiles = t;
    *workgroups = (tcsc::w2_col_tiles(p->cols) + t - 1) / t;
    return TCSC_OK;
}

int tcsc_gpu_plan_set_decode_rows_multi(tcsc_gpu_plan* p, int rows) {
    if (!p) {
        set_error("tcsc_gpu_plan_set_decode_rows_multi: NULL plan");
        return TCSC_E_ARG;
    }
    if (rows != TCSC_DECODE_ROWS_AUTO && (rows < tcsc::kDecodeMaxM || rows > tcsc::kDecodeRowsMax)) {
        set_error("tcsc_gpu_plan_set_decode_rows_multi: rows=%d is neither %d .. %d nor TCSC_DECODE_ROWS_AUTO", rows,
                  tcsc::kDecodeMaxM, tcsc::kDecodeRowsMax);
        return TCSC_E_ARG;
    }
    if (!p->w2) {
        set_error("tcsc_gpu_plan_set_decode_rows_multi: the plan has no 2-bit image (tcsc_gpu_plan_enable_w2, or a packed "
                  "plan)");
        return TCSC_E_ARG;
    }
    p->decode_rows_multi = rows;  // read per gated / grouped call: nothing is allocated, freed or synchronised
    return TCSC_OK;
}

int tcsc_gpu_plan_decode_rows_multi(const tcsc_gpu_plan* p) {
    if (!p) {
        set_error("tcsc_gpu_plan_decode_rows_multi: NULL plan");
        return TCSC_E_ARG;
    }
    return p->decode_rows_multi;
}

int tcsc_gpu_glu_rows_pays(int M, int K, int H, int num_cus) { return glu_rows_pays(M, K, H, num_cus) ? 1 : 0; }
int tcsc_gpu_group_rows_pays(int M, int K, const int* cols, int count, int num_cus) {
    return group_rows_pays(M, K, cols, count, num_cus) ? 1 : 0;
}

int tcsc_gpu_plan_has_i8(const tcsc_gpu_plan* p) {
    if (!p) {
        set_error("tcsc_gpu_plan_has_i8: NULL plan");
        return 0;
    }
    return p->w8 ? 1 : 0;
}

int tcsc_gpu_plan_enable_w2(tcsc_gpu_plan* p, void* stream) {
    if (!p) {
        set_error("tcsc_gpu_plan_enable_w2: NULL plan");
        return TCSC_E_ARG;
    }
    // only beside the int8 image, and only where every i32 sum of k_decode8 stays below 2^31
    if (p->w2 || !p->w8 || p->rows <= 0 || p->rows >= tcsc::kDecodeMaxK || p->cols <= 0) return TCSC_OK;
    DeviceGuard dg(p->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t bytes = tcsc::w2_image_bytes(p->rows, p->cols);
    DevBuf bad;
    if (bad.alloc(sizeof(int)) != hipSuccess || hipMalloc(&p->w2, bytes) != hipSuccess) {
        (void)hipGetLastError();
        p->w2 = nullptr;
        set_error("tcsc_gpu_plan_enable_w2: cannot allocate the 2-bit image (%zu bytes)", bytes);
        return TCSC_E_NOMEM;
    }
    p->w2_bytes = bytes;
    int hbad = 0, rc = TCSC_OK;
    hipError_t e = hipMemsetAsync(bad.p, 0, sizeof(int), st);
    if (e == hipSuccess)
        e = tcsc::decode_build_w2(p->w8, p->cols, p->rows, tcsc::mfma8_ldw(p->rows), p->w2, bad.as<int>(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // the grid rule of k_decode8 (decode_tiles_per_wg) wants the CU count
    if (e == hipSuccess && !p->num_cus)
        e = hipDeviceGetAttribute(&p->num_cus, hipDeviceAttributeMultiprocessorCount, p->device);
    if (e != hipSuccess) rc = hip_fail(e, "tcsc_gpu_plan_enable_w2");
    // a weight that is not -1, 0 or +1 (a duplicated index): no image
    if (rc != TCSC_OK || hbad) free_w2(p);
    return rc;
}

int tcsc_gpu_plan_has_w2(const tcsc_gpu_plan* p) {
    if (!p) {
        set_error("tcsc_gpu_plan_has_w2: NULL plan");
        return 0;
    }
    return p->w2 ? 1 : 0;
}

int tcsc_gpu_w2_image_bytes(int K, int N, size_t* bytes) {
    if (K < 0 || N < 0 || !bytes) {
        set_error("tcsc_gpu_w2_image_bytes: bad arguments (K=%d N=%d)", K, N);
        return TCSC_E_ARG;
    }
    *bytes = tcsc::w2_image_bytes(K, N);
    return TCSC_OK;
}

int tcsc_gpu_decode_pays(int M, int K, int N, long long nnz) { return decode_pays(M, K, N, nnz) ? 1 : 0; }

// tcsc_gpu_sgemm_i8_out with (NULL, TCSC_Y_F32)
int tcsc_gpu_sgemm_i8(const tcsc_gpu_plan* p, const void* dXq, const float* dScale, const float* dB, float* dY, int M,
                      int ldy, int variant, float a, void* stream) {
    return sgemm_entry(p, make_call(dXq, kI8, dScale, dB, YOut{dY, kYF32, nullptr}, M, ldy, variant, a, stream));
}

// ---- the typed Y and the column scales of the int8 calls -------
// what the _out calls check on top of the calls they extend, ahead of any HIP call
static int out_args(const char* who, const tcsc_gpu_plan* p, const float* dB, const void* dY, int ytype) {
    if (ytype != TCSC_Y_F32 && ytype != TCSC_Y_BF16) {
        set_error("%s: ytype=%d is neither TCSC_Y_F32 (0) nor TCSC_Y_BF16 (1)", who, ytype);
        return TCSC_E_ARG;
    }
    if (!p) {
        set_error("%s: NULL plan", who);
        return TCSC_E_ARG;
    }
    if (!dY || !dB) {
        set_error("%s: NULL %s", who, !dY ? "dY" : "dB");
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}

int tcsc_gpu_sgemm_i8_out(const tcsc_gpu_plan* p, const void* dXq, const float* dScale, const float* dColScale,
                          const float* dB, void* dY, int ytype, int M, int ldy, int variant, float a, void* stream) {
    const char* who = "tcsc_gpu_sgemm_i8_out";
    const int rc = out_args(who, p, dB, dY, ytype);
    if (rc != TCSC_OK) return rc;
    return sgemm_entry(p, make_call(dXq, kI8, dScale, dB, y_out(dY, ytype, dColScale), M, ldy, variant, a, stream, who));
}

// the plain quantizer of an fp32 or bf16 X (TCSC_X_F32 / TCSC_X_BF16), under the name of its entry point
static_assert(TCSC_X_F32 == kF32 && TCSC_X_BF16 == kBf16, "the public X types are the internal ones");
static int quantize_rows(int xtype, const void* dX, int M, int K, void* dXq, float* dScale, void* stream) {
    const char* who = xtype == TCSC_X_BF16 ? "tcsc_gpu_quantize_rows_i8_bf16" : "tcsc_gpu_quantize_rows_i8";
    if (M < 0 || K < 0) {
        set_error("%s: bad arguments (M=%d K=%d)", who, M, K);
        return TCSC_E_ARG;
    }
    if (M == 0) return TCSC_OK;
    if (!dScale || (K > 0 && (!dX || !dXq))) {
        set_error("%s: NULL device pointer", who);
        return TCSC_E_ARG;
    }
    HIP_TRY(tcsc::quantize_rows_i8(dX, xtype, nullptr, M, K, static_cast<int8_t*>(dXq), dScale,
                                   static_cast<hipStream_t>(stream)));
    return TCSC_OK;
}

int tcsc_gpu_quantize_rows_i8(const float* dX, int M, int K, void* dXq, float* dScale, void* stream) {
    return quantize_rows(TCSC_X_F32, dX, M, K, dXq, dScale, stream);
}

int tcsc_gpu_quantize_rows_i8_bf16(const void* dX_bf16, int M, int K, void* dXq, float* dScale, void* stream) {
    return quantize_rows(TCSC_X_BF16, dX_bf16, M, K, dXq, dScale, stream);
}

// ---- the quantizer fused into the int8 decode call -------------
// The default rule, host arithmetic.  The fused kernel saves the quantizer's
// launch and its int8 copy; it pays by every workgroup reading all of X twice
// (the row maxima, then the values it quantizes) and quantizing the M K values
// itself.  The byte count put fp32 behind bf16; measured (profiles/q8_bench.json,
// §20) the type hardly matters and the line runs along the values all
// workgroups quantize together: fusing wins up to 2^23 of them (M = 2 at 8192^2,
// M = 4 at 4096^2) and at no M above 4, from where the staging takes a second,
// unprefetched pass of loads per block.
static constexpr int kQFuseMaxM = 4;
static constexpr long long kQFuseValues = 1LL << 23;
// the form of the rule, here and for the norm (below): W M K <= values for 1 <= M <= max_M, W the launch's workgroups
static bool fuse_pays(int M, int K, int N, int xtype, int max_M, long long values) {
    if (M < 1 || M > max_M || K < 1 || N < 1 || (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16)) return false;
    const int T = tcsc::decode_tiles_per_wg(M, N, 0);  // the grid on a 256-CU chip
    const long long wgs = (tcsc::w2_col_tiles(N) + T - 1) / T;
    return wgs * M * K <= values;
}
// $TCSC_QFUSE, read per call: 0 never fuses, 1 fuses on every decode route, unset the rule
static int qfuse_knob() {
    const char* e = std::getenv("TCSC_QFUSE");
    if (!e || !*e) return -1;
    return std::atoi(e) != 0 ? 1 : 0;
}
// The RMSNorm in front of the quantizer: gamma (null = ones) and
// eps of a tcsc_gpu_sgemm_q8_norm call, and the rule for fusing all three steps.
// Every fused workgroup sweeps all of X three times (the squares, the maxima of
// xn, the values it quantizes) where §20's sweeps it twice, and the launch it
// saves is the norm form of the quantizer, which reads a row once and costs
// little more than the plain one.  The rule has the plain one's form (fuse_pays), W M K <=
// kNFuseValues for 1 <= M <= kNFuseMaxM with W the launch's workgroups, and the
// fit to profiles/norm_bench.json is the empty set: of the 40 decode points the
// fused call was faster than the two launches beyond the run's spread only at a
// few of M <= 2 with bf16 x (4096^2, 6912 x 2560: 6 % at the most) and slower
// or level at all others, with losses at M = 1, bf16 (8192^2, 2560 x 6912) at a
// W M K between those of the wins: no bound on W M K separates them, and the
// rule must be 0 wherever the fused call lost.  So kNFuseMaxM = 0: the answer
// is 0 everywhere, and $TCSC_QFUSE=1 is how the fused form runs.
static constexpr int kNFuseMaxM = 0;
static constexpr long long kNFuseValues = 0;
static bool q8_fuse_pays(int M, int K, int N, int xtype, bool norm) {
    return norm ? fuse_pays(M, K, N, xtype, kNFuseMaxM, kNFuseValues) : fuse_pays(M, K, N, xtype, kQFuseMaxM, kQFuseValues);
}
// the int8 route of M rows on the plan as it stands, and whether a q8 call of this X type (norm: a
// q8_norm call) fuses on it
static Route route_q8(const tcsc_gpu_plan* p, int M, int xtype, bool* fused, bool norm) {
    const Route r = route_call(p, M, kI8, p->ws_bytes, RoutePins());
    *fused = false;
    if (r.path == TCSC_PATH_DECODE && has_decode(p, M, kI8) && M <= tcsc::kDecodeMaxM) {  // never fused above 16 rows
        const int knob = qfuse_knob();
        *fused = knob >= 0 ? knob == 1 : q8_fuse_pays(M, p->rows, p->cols, xtype, norm);
    }
    return r;
}

int tcsc_gpu_quant_fuse_pays(int M, int K, int N, int xtype) { return q8_fuse_pays(M, K, N, xtype, false) ? 1 : 0; }

static int launch_info_q8(const char* who, const tcsc_gpu_plan* p, int M, int xtype, bool norm, int* path, int* slices,
                          int* fused) {
    if (!p || M < 0 || !path || !slices || !fused || (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16)) {
        set_error("%s: bad arguments (M=%d xtype=%d)", who, M, xtype);
        return TCSC_E_ARG;
    }
    bool f = false;
    const Route r = route_q8(p, M, xtype, &f, norm);
    *path = r.path;
    *slices = r.slices;
    *fused = f ? 1 : 0;
    return TCSC_OK;
}

int tcsc_gpu_launch_info_q8(const tcsc_gpu_plan* p, int M, int xtype, int* path, int* slices, int* fused) {
    return launch_info_q8("tcsc_gpu_launch_info_q8", p, M, xtype, false, path, slices, fused);
}

// The q8 calls: c is the call as received (X of TCSC_X_F32 / TCSC_X_BF16; c.who names it), dXq the
// caller's scratch for the quantized X and dScale where the row scales go.  `inner`: the name the
// int8 call behind an unfused route gives itself (null: tcsc_gpu_sgemm_i8).  `norm`: the RMSNorm of a
// tcsc_gpu_sgemm_q8_norm call in front of the quantizer (null: none).
static int sgemm_q8_impl(const tcsc_gpu_plan* p, const Call& c, const char* inner, void* dXq, float* dScale,
                         const RmsNorm* norm = nullptr) {
    const char* who = c.who;
    const int M = c.M, xtype = c.xtype;
    if (!p || M < 0 || c.ldy < p->cols || !valid_variant(c.variant) || (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16)) {
        set_error("%s: bad arguments (M=%d ldy=%d variant=%d xtype=%d)", who, M, c.ldy, c.variant, xtype);
        return TCSC_E_ARG;
    }
    if (M == 0) return TCSC_OK;
    if (!dScale || !c.B || !c.y.Y || (!c.X && p->rows > 0)) {
        set_error("%s: NULL device pointer", who);
        return TCSC_E_ARG;
    }
    bool fused = false;
    if (p->cols > 0) {
        const int path = route_q8(p, M, xtype, &fused, norm != nullptr).path;
        if (refuse_out(who, path, c.y, M) || refuse_res(who, path, c.R, M)) return TCSC_E_ARG;
    }
    if (!fused) {  // the quantizer into the caller's scratch, then the int8 call as it is: two or three launches
        if (!dXq && p->rows > 0) {
            set_error("%s: NULL dXq on a route that is not fused (M=%d)", who, M);
            return TCSC_E_ARG;
        }
        const int rc = norm ? tcsc_gpu_quantize_rows_i8_norm(c.X, xtype, norm->gamma, norm->eps, M, p->rows, dXq, dScale,
                                                             c.stream)
                            : quantize_rows(xtype, c.X, M, p->rows, dXq, dScale, c.stream);
        if (rc != TCSC_OK) return rc;
        Call q = c;  // the same call on the quantized X
        q.X = dXq;
        q.xtype = kI8;
        q.xscale = dScale;
        q.who = inner;
        return sgemm_entry(p, q);
    }
    const_cast<tcsc_gpu_plan*>(p)->staged_M = -1;  // as every tcsc_gpu_sgemm* does
    HIP_TRY(tcsc::decode_gemm(tcsc::DecodeX{c.X, xtype, dScale, norm}, p->w2, p->rows, M, p->cols, i8_epi(c), p->num_cus,
                              static_cast<hipStream_t>(c.stream)));
    return TCSC_OK;
}

// tcsc_gpu_sgemm_q8_out with (NULL, TCSC_Y_F32)
int tcsc_gpu_sgemm_q8(const tcsc_gpu_plan* p, const void* dX, int xtype, void* dXq, float* dScale, const float* dB,
                      float* dY, int M, int ldy, int variant, float a, void* stream) {
    return sgemm_q8_impl(p, make_call(dX, xtype, nullptr, dB, YOut{dY, kYF32, nullptr}, M, ldy, variant, a, stream,
                                      "tcsc_gpu_sgemm_q8"),
                         nullptr, dXq, dScale);
}

int tcsc_gpu_sgemm_q8_out(const tcsc_gpu_plan* p, const void* dX, int xtype, void* dXq, float* dScale,
                          const float* dColScale, const float* dB, void* dY, int ytype, int M, int ldy, int variant,
                          float a, void* stream) {
    const char* who = "tcsc_gpu_sgemm_q8_out";
    const int rc = out_args(who, p, dB, dY, ytype);
    if (rc != TCSC_OK) return rc;
    return sgemm_q8_impl(p, make_call(dX, xtype, nullptr, dB, y_out(dY, ytype, dColScale), M, ldy, variant, a, stream, who),
                         who, dXq, dScale);
}

// ---- RMSNorm in the int8 call ----------------------------------
// what the norm calls check on top of the calls they extend, ahead of any HIP call
static int norm_args(const char* who, int xtype, float eps, int K) {
    if (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16) {
        set_error("%s: xtype=%d is neither TCSC_X_F32 (0) nor TCSC_X_BF16 (1)", who, xtype);
        return TCSC_E_ARG;
    }
    if (!std::isfinite(eps) || !(eps > 0.0f)) {
        set_error("%s: eps=%g is not a finite number > 0", who, (double)eps);
        return TCSC_E_ARG;
    }
    if (K < 1) {
        set_error("%s: K=%d < 1", who, K);
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}

int tcsc_gpu_rmsnorm_rows(const void* dX, int xtype, const float* dGamma, float eps, int M, int K, float* dXn,
                          float* dRinv, void* stream) {
    const char* who = "tcsc_gpu_rmsnorm_rows";
    const int rc = norm_args(who, xtype, eps, K);
    if (rc != TCSC_OK) return rc;
    if (M < 0 || !dXn || (M > 0 && !dX)) {
        set_error("%s: %s", who, M < 0 ? "M < 0" : !dXn ? "NULL dXn" : "NULL dX");
        return TCSC_E_ARG;
    }
    if (M == 0) return TCSC_OK;
    HIP_TRY(tcsc::rmsnorm_rows(dX, xtype == TCSC_X_BF16, dGamma, eps, M, K, dXn, dRinv,
                               static_cast<hipStream_t>(stream)));
    return TCSC_OK;
}

int tcsc_gpu_quantize_rows_i8_norm(const void* dX, int xtype, const float* dGamma, float eps, int M, int K, void* dXq,
                                   float* dScale, void* stream) {
    const char* who = "tcsc_gpu_quantize_rows_i8_norm";
    const int rc = norm_args(who, xtype, eps, K);
    if (rc != TCSC_OK) return rc;
    if (M < 0) {
        set_error("%s: M < 0", who);
        return TCSC_E_ARG;
    }
    if (M == 0) return TCSC_OK;
    if (!dX || !dXq || !dScale) {
        set_error("%s: NULL device pointer", who);
        return TCSC_E_ARG;
    }
    const RmsNorm norm{dGamma, eps};
    HIP_TRY(tcsc::quantize_rows_i8(dX, xtype, &norm, M, K, static_cast<int8_t*>(dXq), dScale,
                                   static_cast<hipStream_t>(stream)));
    return TCSC_OK;
}

int tcsc_gpu_norm_fuse_pays(int M, int K, int N, int xtype) { return q8_fuse_pays(M, K, N, xtype, true) ? 1 : 0; }

int tcsc_gpu_launch_info_q8_norm(const tcsc_gpu_plan* p, int M, int xtype, int* path, int* slices, int* fused) {
    return launch_info_q8("tcsc_gpu_launch_info_q8_norm", p, M, xtype, true, path, slices, fused);
}

int tcsc_gpu_sgemm_q8_norm(const tcsc_gpu_plan* p, const void* dX, int xtype, const float* dGamma, float eps, void* dXq,
                           float* dScale, const float* dColScale, const float* dB, void* dY, int ytype, int M, int ldy,
                           int variant, float a, void* stream) {
    const char* who = "tcsc_gpu_sgemm_q8_norm";
    int rc = norm_args(who, xtype, eps, p ? p->rows : 1);  // K is the plan's: a NULL plan is out_args'
    if (rc != TCSC_OK) return rc;
    rc = out_args(who, p, dB, dY, ytype);
    if (rc != TCSC_OK) return rc;
    const RmsNorm norm{dGamma, eps};
    return sgemm_q8_impl(p, make_call(dX, xtype, nullptr, dB, y_out(dY, ytype, dColScale), M, ldy, variant, a, stream, who),
                         who, dXq, dScale, &norm);
}

// ---- the residual add in the epilogue ---------------------------
// Y = R + X W: the _out and _q8_out / _q8_norm calls without PReLU, with R[m * ldr + j] (of Y's type)
// added to the value in the epilogue of the decode and MFMA routes.  What the calls check on top of
// out_args, ahead of any HIP call and in this order: a NULL dR, ldr < cols, and an R that is Y at
// another pitch than Y's.
static int res_args(const char* who, const tcsc_gpu_plan* p, const float* dB, const void* dR, int ldr, const void* dY,
                    int ytype, int ldy) {
    const int rc = out_args(who, p, dB, dY, ytype);
    if (rc != TCSC_OK) return rc;
    if (!dR) {
        set_error("%s: NULL dR", who);
        return TCSC_E_ARG;
    }
    if (ldr < p->cols) {
        set_error("%s: ldr=%d < cols=%d", who, ldr, p->cols);
        return TCSC_E_ARG;
    }
    if (dR == dY && ldr != ldy) {
        set_error("%s: dR == dY (in place) with ldr=%d != ldy=%d", who, ldr, ldy);
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}

int tcsc_gpu_sgemm_i8_res(const tcsc_gpu_plan* p, const void* dXq, const float* dScale, const float* dColScale,
                          const float* dB, const void* dR, int ldr, void* dY, int ytype, int M, int ldy, void* stream) {
    const char* who = "tcsc_gpu_sgemm_i8_res";
    const int rc = res_args(who, p, dB, dR, ldr, dY, ytype, ldy);
    if (rc != TCSC_OK) return rc;
    Call c = make_call(dXq, kI8, dScale, dB, y_out(dY, ytype, dColScale), M, ldy, TCSC_VARIANT_BASIC, 0.f, stream, who);
    c.R = dR;
    c.ldr = ldr;
    return sgemm_entry(p, c);
}

int tcsc_gpu_sgemm_q8_res(const tcsc_gpu_plan* p, const void* dX, int xtype, const float* dGamma, float eps, void* dXq,
                          float* dScale, const float* dColScale, const float* dB, const void* dR, int ldr, void* dY,
                          int ytype, int M, int ldy, void* stream) {
    const char* who = "tcsc_gpu_sgemm_q8_res";
    if (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16) {
        set_error("%s: xtype=%d is neither TCSC_X_F32 (0) nor TCSC_X_BF16 (1)", who, xtype);
        return TCSC_E_ARG;
    }
    const bool has_norm = eps != 0.0f;  // eps == 0 exactly: no norm in front (tcsc_gpu_sgemm_q8_glu's convention)
    if (!has_norm && dGamma) {
        set_error("%s: dGamma given with eps == 0 (no norm): pass the norm's eps, or a NULL dGamma", who);
        return TCSC_E_ARG;
    }
    int rc = has_norm ? norm_args(who, xtype, eps, p ? p->rows : 1) : TCSC_OK;
    if (rc != TCSC_OK) return rc;
    rc = res_args(who, p, dB, dR, ldr, dY, ytype, ldy);
    if (rc != TCSC_OK) return rc;
    const RmsNorm norm{dGamma, eps};
    Call c = make_call(dX, xtype, nullptr, dB, y_out(dY, ytype, dColScale), M, ldy, TCSC_VARIANT_BASIC, 0.f, stream, who);
    c.R = dR;
    c.ldr = ldr;
    return sgemm_q8_impl(p, c, who, dXq, dScale, has_norm ? &norm : nullptr);
}

// ---- the gated FFN call -----------------------------------------
// Y = act(X Wg) (X Wu) on two plans with the 2-bit image and the same K and H.  The route is fixed by
// M and, from 17 to 64 rows, the two plans' decode_rows_multi setting (glu_decodes, §28), whatever the cost
// models, $TCSC_PATH or $TCSC_DECODE say: up to 16 rows, and up to 64 where the setting admits M, the one gated
// decode launch, otherwise k_pack8 once and k_gemm8w2 twice on the gate plan's workspace -- the gate half into the
// caller's G through the plain epilogue, the up half with the gated one.
static_assert(TCSC_GLU_RELU2 == tcsc::kGluRelu2 && TCSC_GLU_SILU == tcsc::kGluSilu, "the public gate activations are i8_glu's");

// The fusing rule of the gated q8 call: §20's (and with the norm §22's, which is 0 everywhere) with the
// gated launch's own workgroup count.
static bool glu_fuse_pays(int M, int K, int N, int xtype, bool norm) {
    const int max_M = norm ? kNFuseMaxM : kQFuseMaxM;
    const long long values = norm ? kNFuseValues : kQFuseValues;
    if (M < 1 || M > max_M || K < 1 || N < 1 || (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16)) return false;
    const int TG = tcsc::decode_glu_tiles_per_wg(M, N, 0);  // the grid on a 256-CU chip
    const long long wgs = (tcsc::w2_col_tiles(N) + TG - 1) / TG;
    return wgs * M * K <= values;
}
int tcsc_gpu_glu_fuse_pays(int M, int K, int N, int xtype, int norm) { return glu_fuse_pays(M, K, N, xtype, norm != 0) ? 1 : 0; }

// what every gated entry point checks of its plans, ahead of any HIP call
static int glu_plans(const char* who, const tcsc_gpu_plan* gate, const tcsc_gpu_plan* up) {
    if (!gate || !up) {
        set_error("%s: NULL %s plan", who, !gate ? "gate" : "up");
        return TCSC_E_ARG;
    }
    if (!gate->w2 || !up->w2) {
        set_error("%s: the %s plan has no 2-bit image (a packed plan, or tcsc_gpu_plan_enable_w2 on an ordinary one)", who,
                  !gate->w2 ? "gate" : "up");
        return TCSC_E_ARG;
    }
    if (gate->rows != up->rows || gate->cols != up->cols || gate->device != up->device) {
        set_error("%s: the gate plan is K=%d x cols=%d on device %d and the up plan K=%d x cols=%d on device %d", who,
                  gate->rows, gate->cols, gate->device, up->rows, up->cols, up->device);
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}
static int glu_args(const char* who, const tcsc_gpu_plan* gate, const tcsc_gpu_plan* up, const float* dBG,
                    const float* dBU, const void* dY, int ytype, int act) {
    if (ytype != TCSC_Y_F32 && ytype != TCSC_Y_BF16) {
        set_error("%s: ytype=%d is neither TCSC_Y_F32 (0) nor TCSC_Y_BF16 (1)", who, ytype);
        return TCSC_E_ARG;
    }
    if (act != TCSC_GLU_RELU2 && act != TCSC_GLU_SILU) {
        set_error("%s: act=%d is neither TCSC_GLU_RELU2 (0) nor TCSC_GLU_SILU (1)", who, act);
        return TCSC_E_ARG;
    }
    const int rc = glu_plans(who, gate, up);
    if (rc != TCSC_OK) return rc;
    if (!dY || !dBG || !dBU) {
        set_error("%s: NULL %s", who, !dY ? "dY" : !dBG ? "dBG" : "dBU");
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}
// the MFMA workspace of M rows of a gated call: the int8 call's on the gate plan (the slabs serve both GEMMs in turn)
static size_t glu_ws_bytes(const tcsc_gpu_plan* gate, int M) {
    return mfma_ws(kI8, std::min(M, kMaxLaunchRows), gate->rows, gate->cols).bytes;
}

// A gated call on an int8 X (c.xtype == kI8; c.glu.up set; the plans and pointers checked by glu_args).
static int sgemm_glu_i8(const tcsc_gpu_plan* gate, const Call& c) {
    const char* who = c.who;
    const tcsc_gpu_plan* up = c.glu.up;
    const int M = c.M, K = gate->rows, H = gate->cols;
    if (M < 0 || c.ldy < H) {
        set_error("%s: bad arguments (M=%d ldy=%d cols=%d)", who, M, c.ldy, H);
        return TCSC_E_ARG;
    }
    if (M == 0 || H == 0) return TCSC_OK;
    if (!c.X) {
        set_error("%s: NULL X", who);
        return TCSC_E_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(c.stream);
    I8Epi eg, eu;  // the two halves: the gate's own epilogue, and the up half's with the gate beside it
    eg.rscale = eu.rscale = c.xscale;
    eg.B = c.B;
    eg.y = YOut{c.glu.G, kYF32, c.y.cscale};
    eg.ldy = c.glu.ldg;
    eu.B = c.glu.B;
    eu.y = YOut{c.y.Y, c.y.ytype, c.glu.cscale};
    eu.ldy = c.ldy;
    eu.act = c.glu.act;
    if (glu_decodes(gate, up, M)) {  // TCSC_PATH_DECODE: one launch, G untouched
        HIP_TRY(tcsc::decode_glu(tcsc::DecodeX{c.X, kI8, nullptr, nullptr}, gate->w2, up->w2, K, M, H, eg, eu, gate->num_cus,
                                 st));
        return TCSC_OK;
    }
    if (!c.glu.G) {
        set_error("%s: NULL dG on the MFMA route (M=%d)", who, M);
        return TCSC_E_ARG;
    }
    if (gate->ws_bytes < glu_ws_bytes(gate, M)) {  // grown on first use, as every tcsc_gpu_sgemm* does
        const int rc = tcsc_gpu_plan_reserve(const_cast<tcsc_gpu_plan*>(gate), M);
        if (rc != TCSC_OK) return rc;
    }
    const_cast<tcsc_gpu_plan*>(gate)->staged_M = -1;
    for (int r0 = 0; r0 < M; r0 += kMaxLaunchRows) {  // pieces of at most kMaxLaunchRows rows on one workspace
        const Call q = c.rows(r0, std::min(kMaxLaunchRows, M - r0), K, 1);
        const MfmaWs w = mfma_ws(kI8, q.M, K, H);
        if (!gate->ws || gate->ws_bytes < w.bytes) {
            set_error("%s: workspace of %zu bytes < %zu needed for M=%d", who, gate->ws ? gate->ws_bytes : (size_t)0, w.bytes,
                      q.M);
            return TCSC_E_ARG;
        }
        char* base = reinterpret_cast<char*>(gate->ws);
        int8_t* x8 = reinterpret_cast<int8_t*>(base);
        int* slabs = reinterpret_cast<int*>(base + w.slabs_off);
        const size_t slab_bytes = gate->ws_bytes - w.slabs_off;
        const int ld8 = tcsc::mfma8_ldw(K);
        eg.rscale = eu.rscale = q.xscale;
        eg.y.Y = q.glu.G;
        eu.y.Y = q.y.Y;
        eu.G = q.glu.G;
        eu.ldg = q.glu.ldg;
        HIP_TRY(tcsc::mfma8_pack_x(static_cast<const int8_t*>(q.X), q.M, K, x8, ld8, st));
        HIP_TRY(tcsc::mfma8_gemm_w2(x8, gate->w2, ld8, K, q.M, H, eg, slabs, slab_bytes, st));
        HIP_TRY(tcsc::mfma8_gemm_w2(x8, up->w2, ld8, K, q.M, H, eu, slabs, slab_bytes, st));
    }
    return TCSC_OK;
}

static Call glu_call(const char* who, const void* X, int xtype, const float* xscale, const tcsc_gpu_plan* up,
                     const float* cg, const float* bg, const float* cu, const float* bu, float* dG, void* dY, int ytype,
                     int M, int ldy, int H, int act, void* stream) {
    Call c = make_call(X, xtype, xscale, bg, y_out(dY, ytype, cg), M, ldy, TCSC_VARIANT_BASIC, 0.f, stream, who);
    c.glu = tcsc::GluUp{up, cu, bu, dG, H, act};
    return c;
}

int tcsc_gpu_sgemm_i8_glu(const tcsc_gpu_plan* gate, const tcsc_gpu_plan* up, const void* dXq, const float* dScale,
                          const float* dColScaleG, const float* dBG, const float* dColScaleU, const float* dBU, float* dG,
                          void* dY, int ytype, int M, int ldy, int act, void* stream) {
    const char* who = "tcsc_gpu_sgemm_i8_glu";
    const int rc = glu_args(who, gate, up, dBG, dBU, dY, ytype, act);
    if (rc != TCSC_OK) return rc;
    return sgemm_glu_i8(gate, glu_call(who, dXq, kI8, dScale, up, dColScaleG, dBG, dColScaleU, dBU, dG, dY, ytype, M, ldy,
                                       gate->cols, act, stream));
}

// whether a gated q8 call of M rows fuses the quantizer (norm: and the norm) into the decode launch
static bool glu_fused(int M, int K, int H, int xtype, bool norm) {
    if (M < 1 || M > tcsc::kDecodeMaxM) return false;
    const int knob = qfuse_knob();
    return knob >= 0 ? knob == 1 : glu_fuse_pays(M, K, H, xtype, norm);
}

int tcsc_gpu_sgemm_q8_glu(const tcsc_gpu_plan* gate, const tcsc_gpu_plan* up, const void* dX, int xtype,
                          const float* dGamma, float eps, void* dXq, float* dScale, const float* dColScaleG,
                          const float* dBG, const float* dColScaleU, const float* dBU, float* dG, void* dY, int ytype,
                          int M, int ldy, int act, void* stream) {
    const char* who = "tcsc_gpu_sgemm_q8_glu";
    if (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16) {
        set_error("%s: xtype=%d is neither TCSC_X_F32 (0) nor TCSC_X_BF16 (1)", who, xtype);
        return TCSC_E_ARG;
    }
    const bool has_norm = eps != 0.0f;  // eps == 0 exactly: no norm in front
    if (!has_norm && dGamma) {
        set_error("%s: dGamma given with eps == 0 (no norm): pass the norm's eps, or a NULL dGamma", who);
        return TCSC_E_ARG;
    }
    int rc = has_norm ? norm_args(who, xtype, eps, gate ? gate->rows : 1) : TCSC_OK;
    if (rc != TCSC_OK) return rc;
    rc = glu_args(who, gate, up, dBG, dBU, dY, ytype, act);
    if (rc != TCSC_OK) return rc;
    const int K = gate->rows, H = gate->cols;
    if (M < 0 || ldy < H) {
        set_error("%s: bad arguments (M=%d ldy=%d cols=%d)", who, M, ldy, H);
        return TCSC_E_ARG;
    }
    if (M == 0 || H == 0) return TCSC_OK;
    if (!dX || !dScale) {
        set_error("%s: NULL %s", who, !dX ? "dX" : "dScale");
        return TCSC_E_ARG;
    }
    const RmsNorm norm{dGamma, eps};
    Call c = glu_call(who, dX, xtype, nullptr, up, dColScaleG, dBG, dColScaleU, dBU, dG, dY, ytype, M, ldy, H, act, stream);
    if (glu_fused(M, K, H, xtype, has_norm)) {
        I8Epi eg, eu;
        eg.B = dBG;
        eg.y.cscale = dColScaleG;
        eu.B = dBU;
        eu.y = c.y;
        eu.y.cscale = dColScaleU;
        eu.ldy = ldy;
        eu.act = act;
        HIP_TRY(tcsc::decode_glu(tcsc::DecodeX{dX, xtype, dScale, has_norm ? &norm : nullptr}, gate->w2, up->w2, K, M, H, eg,
                                 eu, gate->num_cus, static_cast<hipStream_t>(stream)));
        return TCSC_OK;
    }
    if (!dXq) {
        set_error("%s: NULL dXq on a route that is not fused (M=%d)", who, M);
        return TCSC_E_ARG;
    }
    if (!glu_decodes(gate, up, M) && !dG) {  // ahead of the quantizer's launch
        set_error("%s: NULL dG on the MFMA route (M=%d)", who, M);
        return TCSC_E_ARG;
    }
    rc = has_norm ? tcsc_gpu_quantize_rows_i8_norm(dX, xtype, dGamma, eps, M, K, dXq, dScale, stream)
                  : quantize_rows(xtype, dX, M, K, dXq, dScale, stream);
    if (rc != TCSC_OK) return rc;
    c.X = dXq;
    c.xtype = kI8;
    c.xscale = dScale;
    return sgemm_glu_i8(gate, c);
}

int tcsc_gpu_launch_info_glu(const tcsc_gpu_plan* gate, const tcsc_gpu_plan* up, int M, int xtype, int* path, int* slices,
                             int* fused) {
    const char* who = "tcsc_gpu_launch_info_glu";
    if (M < 0 || !path || !slices || !fused || (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16)) {
        set_error("%s: bad arguments (M=%d xtype=%d)", who, M, xtype);
        return TCSC_E_ARG;
    }
    const int rc = glu_plans(who, gate, up);
    if (rc != TCSC_OK) return rc;
    const bool decode = glu_decodes(gate, up, M);
    *path = decode ? TCSC_PATH_DECODE : TCSC_PATH_MFMA;
    *slices = decode ? 1 : tcsc::mfma8_slices(std::min(M, kMaxLaunchRows), gate->cols, gate->rows);
    *fused = glu_fused(M, gate->rows, gate->cols, xtype, false) ? 1 : 0;
    return TCSC_OK;
}

// ---- the grouped call -------------------------------------------
// Up to TCSC_GROUP_MAX plans with the 2-bit image and one K on one X: member i gets the bits of
// tcsc_gpu_sgemm_i8_out on its own plan.  The route is fixed as the gated call's (group_plans_decode, §28):
// up to 16 rows, and up to 64 where every member's decode_rows_multi setting admits M, one grouped decode launch,
// otherwise k_pack8 once (into the first member's workspace) and k_gemm8w2
// once per member, each GEMM's slabs in its own plan's workspace.
static_assert(TCSC_GROUP_MAX == tcsc::kGroupMax, "the public group size is the launch table's");

// The fusing rule of the grouped q8 call: §20's with the grouped launch's own workgroup count.  The
// grouped launch has no norm form, so with the norm the answer is 0 (as §22's rule is everywhere).
static bool group_fuse_pays(int M, int K, const int* cols, int count, int xtype, bool norm) {
    if (norm || M < 1 || M > kQFuseMaxM || K < 1 || !cols || count < 1 || count > TCSC_GROUP_MAX ||
        (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16))
        return false;
    for (int i = 0; i < count; ++i)
        if (cols[i] < 1) return false;
    const int T = tcsc::decode_group_tiles_per_wg(M, cols, count, 0);  // the grid on a 256-CU chip
    return tcsc::decode_group_wgs(cols, count, T) * M * K <= kQFuseValues;
}
int tcsc_gpu_group_fuse_pays(int M, int K, const int* cols, int count, int xtype, int norm) {
    return group_fuse_pays(M, K, cols, count, xtype, norm != 0) ? 1 : 0;
}

// what every grouped entry point checks of its group, ahead of any HIP call (group_plans' outputs: with the
// members' dB, dY and ldy)
static int group_members(const char* who, const tcsc_gpu_group_member* m, int count) {
    if (count < 1 || count > TCSC_GROUP_MAX) {
        set_error("%s: count=%d is outside 1 .. %d (TCSC_GROUP_MAX)", who, count, TCSC_GROUP_MAX);
        return TCSC_E_ARG;
    }
    if (!m) {
        set_error("%s: NULL members", who);
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}
static int group_plans(const char* who, const tcsc_gpu_group_member* m, int count, bool outputs) {
    for (int i = 0; i < count; ++i) {
        if (!m[i].plan || (outputs && (!m[i].dB || !m[i].dY))) {
            set_error("%s: member %d: NULL %s", who, i, !m[i].plan ? "plan" : !m[i].dB ? "dB" : "dY");
            return TCSC_E_ARG;
        }
    }
    for (int i = 0; i < count; ++i) {
        if (!m[i].plan->w2) {
            set_error("%s: member %d: the plan has no 2-bit image (a packed plan, or tcsc_gpu_plan_enable_w2 on an ordinary "
                      "one)", who, i);
            return TCSC_E_ARG;
        }
    }
    for (int i = 1; i < count; ++i) {
        if (m[i].plan->rows != m[0].plan->rows || m[i].plan->device != m[0].plan->device) {
            set_error("%s: member %d: the plan has K=%d on device %d and member 0's K=%d on device %d", who, i,
                      m[i].plan->rows, m[i].plan->device, m[0].plan->rows, m[0].plan->device);
            return TCSC_E_ARG;
        }
    }
    if (!outputs) return TCSC_OK;
    for (int i = 0; i < count; ++i) {
        if (m[i].ldy < m[i].plan->cols) {
            set_error("%s: member %d: ldy=%d < cols=%d", who, i, m[i].ldy, m[i].plan->cols);
            return TCSC_E_ARG;
        }
    }
    return TCSC_OK;
}
static int group_ytype(const char* who, int ytype) {
    if (ytype == TCSC_Y_F32 || ytype == TCSC_Y_BF16) return TCSC_OK;
    set_error("%s: ytype=%d is neither TCSC_Y_F32 (0) nor TCSC_Y_BF16 (1)", who, ytype);
    return TCSC_E_ARG;
}
static int group_xtype(const char* who, int xtype) {
    if (xtype == TCSC_X_F32 || xtype == TCSC_X_BF16) return TCSC_OK;
    set_error("%s: xtype=%d is neither TCSC_X_F32 (0) nor TCSC_X_BF16 (1)", who, xtype);
    return TCSC_E_ARG;
}

// the members of a call in one list: member 0 from the call's own fields, the rest from c.group
struct GroupView {
    int count = 0;
    const tcsc_gpu_plan* plan[TCSC_GROUP_MAX];
    tcsc::DecodeMember m[TCSC_GROUP_MAX];
};
static GroupView group_view(const tcsc_gpu_plan* first, const Call& c) {
    GroupView v;
    for (int i = 0; i <= c.group.count; ++i) {
        const tcsc_gpu_plan* p = i ? c.group.m[i - 1].plan : first;
        if (p->cols == 0) continue;  // nothing to write
        tcsc::DecodeMember& d = v.m[v.count];
        v.plan[v.count++] = p;
        d.w2 = p->w2;
        d.N = p->cols;
        d.e.rscale = c.xscale;
        d.e.B = i ? c.group.m[i - 1].B : c.B;
        d.e.y = i ? c.group.m[i - 1].y : c.y;
        d.e.ldy = i ? c.group.m[i - 1].ldy : c.ldy;
    }
    return v;
}

// a grouped call of M rows takes TCSC_PATH_DECODE: up to 16 rows always, above where every member's plan admits M
// (decode_rows_multi, §28; AUTO asks group_rows_pays on the members that have columns)
static bool group_plans_decode(const tcsc_gpu_plan* const* plan, int count, int M) {
    if (M <= tcsc::kDecodeMaxM) return true;
    if (M > tcsc::kDecodeRowsMax) return false;
    int cols[TCSC_GROUP_MAX], n = 0;
    for (int i = 0; i < count; ++i)
        if (plan[i]->cols > 0) cols[n++] = plan[i]->cols;
    const bool pays = n > 0 && group_rows_pays(M, plan[0]->rows, cols, n, plan[0]->num_cus);
    for (int i = 0; i < count; ++i)
        if (!multi_rows_admits(plan[i], M, pays)) return false;
    return true;
}
static bool group_decodes(const tcsc_gpu_group_member* m, int count, int M) {
    const tcsc_gpu_plan* plan[TCSC_GROUP_MAX];
    for (int i = 0; i < count; ++i) plan[i] = m[i].plan;
    return group_plans_decode(plan, count, M);
}
// the same of a call: member 0 is the call's own plan, the rest c.group's
static bool group_call_decodes(const tcsc_gpu_plan* first, const Call& c) {
    const tcsc_gpu_plan* plan[TCSC_GROUP_MAX];
    plan[0] = first;
    for (int i = 0; i < c.group.count; ++i) plan[i + 1] = c.group.m[i].plan;
    return group_plans_decode(plan, c.group.count + 1, c.M);
}

// A grouped call on an int8 X (c.xtype == kI8; the members checked by group_plans).
static int sgemm_group_i8(const tcsc_gpu_plan* first, const Call& c) {
    const char* who = c.who;
    const int M = c.M, K = first->rows;
    if (M < 0) {
        set_error("%s: bad arguments (M=%d)", who, M);
        return TCSC_E_ARG;
    }
    if (M == 0) return TCSC_OK;
    if (!c.X) {
        set_error("%s: NULL X", who);
        return TCSC_E_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(c.stream);
    if (group_call_decodes(first, c)) {
        const GroupView v = group_view(first, c);  // TCSC_PATH_DECODE: one launch
        if (!v.count) return TCSC_OK;
        HIP_TRY(tcsc::decode_group(tcsc::DecodeX{c.X, kI8, nullptr, nullptr}, v.m, v.count, K, M, first->num_cus, st));
        return TCSC_OK;
    }
    {  // every member's workspace, grown on first use as every tcsc_gpu_sgemm* does
        const GroupView v = group_view(first, c);
        for (int i = 0; i < v.count; ++i) {
            tcsc_gpu_plan* p = const_cast<tcsc_gpu_plan*>(v.plan[i]);
            if (p->ws_bytes < mfma_ws(kI8, std::min(M, kMaxLaunchRows), K, p->cols).bytes) {
                const int rc = tcsc_gpu_plan_reserve(p, M);
                if (rc != TCSC_OK) return rc;
            }
            p->staged_M = -1;
        }
    }
    for (int r0 = 0; r0 < M; r0 += kMaxLaunchRows) {  // pieces of at most kMaxLaunchRows rows on the same workspaces
        const Call q = c.rows(r0, std::min(kMaxLaunchRows, M - r0), K, 1);
        const GroupView v = group_view(first, q);
        if (!v.count) return TCSC_OK;
        const int ld8 = tcsc::mfma8_ldw(K);
        for (int i = 0; i < v.count; ++i) {
            const tcsc_gpu_plan* p = v.plan[i];
            const size_t need = mfma_ws(kI8, q.M, K, p->cols).bytes;
            if (!p->ws || p->ws_bytes < need) {
                set_error("%s: member %d: workspace of %zu bytes < %zu needed for M=%d", who, i,
                          p->ws ? p->ws_bytes : (size_t)0, need, q.M);
                return TCSC_E_ARG;
            }
        }
        int8_t* x8 = reinterpret_cast<int8_t*>(v.plan[0]->ws);  // the packed X of all members' GEMMs
        HIP_TRY(tcsc::mfma8_pack_x(static_cast<const int8_t*>(q.X), q.M, K, x8, ld8, st));
        for (int i = 0; i < v.count; ++i) {
            const tcsc_gpu_plan* p = v.plan[i];
            const MfmaWs w = mfma_ws(kI8, q.M, K, p->cols);  // the slabs where the member's own call has them
            char* base = reinterpret_cast<char*>(p->ws);
            HIP_TRY(tcsc::mfma8_gemm_w2(x8, p->w2, ld8, K, q.M, p->cols, v.m[i].e, reinterpret_cast<int*>(base + w.slabs_off),
                                        p->ws_bytes - w.slabs_off, st));
        }
    }
    return TCSC_OK;
}

static Call group_call(const char* who, const tcsc_gpu_group_member* m, int count, const void* X, int xtype,
                       const float* xscale, int ytype, int M, void* stream) {
    Call c = make_call(X, xtype, xscale, m[0].dB, y_out(m[0].dY, ytype, m[0].dColScale), M, m[0].ldy, TCSC_VARIANT_BASIC,
                       0.f, stream, who);
    c.group.count = count - 1;
    for (int i = 1; i < count; ++i)
        c.group.m[i - 1] = tcsc::GroupRest::Member{m[i].plan, m[i].dB, y_out(m[i].dY, ytype, m[i].dColScale), m[i].ldy};
    return c;
}

int tcsc_gpu_sgemm_i8_group(const tcsc_gpu_group_member* members, int count, const void* dXq, const float* dScale,
                            int ytype, int M, void* stream) {
    const char* who = "tcsc_gpu_sgemm_i8_group";
    int rc = group_members(who, members, count);
    if (rc == TCSC_OK) rc = group_ytype(who, ytype);
    if (rc == TCSC_OK) rc = group_plans(who, members, count, true);
    if (rc != TCSC_OK) return rc;
    return sgemm_group_i8(members[0].plan, group_call(who, members, count, dXq, kI8, dScale, ytype, M, stream));
}

// whether a grouped q8 call of M rows without the norm quantizes inside the decode launch
static bool group_fused(const tcsc_gpu_group_member* m, int count, int M, int xtype) {
    if (M < 1 || M > tcsc::kDecodeMaxM) return false;
    int cols[TCSC_GROUP_MAX], n = 0;
    for (int i = 0; i < count; ++i)
        if (m[i].plan->cols > 0) cols[n++] = m[i].plan->cols;
    if (!n) return false;
    const int knob = qfuse_knob();
    return knob >= 0 ? knob == 1 : group_fuse_pays(M, m[0].plan->rows, cols, n, xtype, false);
}

int tcsc_gpu_sgemm_q8_group(const tcsc_gpu_group_member* members, int count, const void* dX, int xtype,
                            const float* dGamma, float eps, void* dXq, float* dScale, int ytype, int M, void* stream) {
    const char* who = "tcsc_gpu_sgemm_q8_group";
    int rc = group_members(who, members, count);
    if (rc == TCSC_OK) rc = group_ytype(who, ytype);
    if (rc == TCSC_OK) rc = group_xtype(who, xtype);
    if (rc != TCSC_OK) return rc;
    const bool has_norm = eps != 0.0f;  // eps == 0 exactly: no norm in front
    if (has_norm) rc = norm_args(who, xtype, eps, members[0].plan ? members[0].plan->rows : 1);
    if (rc != TCSC_OK) return rc;
    if (!has_norm && dGamma) {
        set_error("%s: dGamma given with eps == 0 (no norm): pass the norm's eps, or a NULL dGamma", who);
        return TCSC_E_ARG;
    }
    rc = group_plans(who, members, count, true);
    if (rc != TCSC_OK) return rc;
    const int K = members[0].plan->rows;
    if (M < 0) {
        set_error("%s: bad arguments (M=%d)", who, M);
        return TCSC_E_ARG;
    }
    if (M == 0) return TCSC_OK;
    if (!dX || !dScale) {
        set_error("%s: NULL %s", who, !dX ? "dX" : "dScale");
        return TCSC_E_ARG;
    }
    Call c = group_call(who, members, count, dX, xtype, nullptr, ytype, M, stream);
    if (!has_norm && group_fused(members, count, M, xtype)) {  // the grouped launch has no norm form
        const GroupView v = group_view(members[0].plan, c);
        HIP_TRY(tcsc::decode_group(tcsc::DecodeX{dX, xtype, dScale, nullptr}, v.m, v.count, K, M, members[0].plan->num_cus,
                                   static_cast<hipStream_t>(stream)));
        return TCSC_OK;
    }
    if (!dXq) {
        set_error("%s: NULL dXq on a route that is not fused (M=%d)", who, M);
        return TCSC_E_ARG;
    }
    rc = has_norm ? tcsc_gpu_quantize_rows_i8_norm(dX, xtype, dGamma, eps, M, K, dXq, dScale, stream)
                  : quantize_rows(xtype, dX, M, K, dXq, dScale, stream);
    if (rc != TCSC_OK) return rc;
    c.X = dXq;
    c.xtype = kI8;
    c.xscale = dScale;
    return sgemm_group_i8(members[0].plan, c);
}

int tcsc_gpu_launch_info_group(const tcsc_gpu_group_member* members, int count, int M, int xtype, int* path, int* slices,
                               int* fused) {
    const char* who = "tcsc_gpu_launch_info_group";
    int rc = group_members(who, members, count);
    if (rc != TCSC_OK) return rc;
    if (M < 0 || !path || !slices || !fused || (xtype != TCSC_X_F32 && xtype != TCSC_X_BF16)) {
        set_error("%s: bad arguments (M=%d xtype=%d)", who, M, xtype);
        return TCSC_E_ARG;
    }
    rc = group_plans(who, members, count, false);
    if (rc != TCSC_OK) return rc;
    const bool decode = group_decodes(members, count, M);
    *path = decode ? TCSC_PATH_DECODE : TCSC_PATH_MFMA;
    for (int i = 0; i < count; ++i)
        slices[i] = decode || members[i].plan->cols == 0
                        ? 1
                        : tcsc::mfma8_slices(std::min(M, kMaxLaunchRows), members[i].plan->cols, members[i].plan->rows);
    *fused = group_fused(members, count, M, xtype) ? 1 : 0;
    return TCSC_OK;
}

int tcsc_gpu_launch_info_glu_decode(const tcsc_gpu_plan* gate, const tcsc_gpu_plan* up, int M, int* row_tiles,
                                    int* col_tiles, long long* workgroups) {
    const char* who = "tcsc_gpu_launch_info_glu_decode";
    if (!row_tiles || !col_tiles || !workgroups) {
        set_error("%s: bad arguments", who);
        return TCSC_E_ARG;
    }
    const int rc = glu_plans(who, gate, up);
    if (rc != TCSC_OK) return rc;
    if (M < 1 || M > tcsc::kDecodeRowsMax) {
        set_error("%s: no decode launch of M=%d rows (1 .. %d)", who, M, tcsc::kDecodeRowsMax);
        return TCSC_E_ARG;
    }
    const int rt = tcsc::decode_row_tiles(M);
    const int t = rt > 1 ? tcsc::decode_glu_rows_tiles_per_wg(M, gate->cols, gate->num_cus)
                         : tcsc::decode_glu_tiles_per_wg(M, gate->cols, gate->num_cus);
    *row_tiles = rt;
    *col_tiles = t;
    *workgroups = (tcsc::w2_col_tiles(gate->cols) + t - 1) / t;
    return TCSC_OK;
}

int tcsc_gpu_launch_info_group_decode(const tcsc_gpu_group_member* members, int count, int M, int* row_tiles,
                                      int* col_tiles, long long* workgroups) {
    const char* who = "tcsc_gpu_launch_info_group_decode";
    int rc = group_members(who, members, count);
    if (rc != TCSC_OK) return rc;
    if (!row_tiles || !col_tiles || !workgroups) {
        set_error("%s: bad arguments", who);
        return TCSC_E_ARG;
    }
    rc = group_plans(who, members, count, false);
    if (rc != TCSC_OK) return rc;
    if (M < 1 || M > tcsc::kDecodeRowsMax) {
        set_error("%s: no decode launch of M=%d rows (1 .. %d)", who, M, tcsc::kDecodeRowsMax);
        return TCSC_E_ARG;
    }
    int cols[TCSC_GROUP_MAX], n = 0;  // the launch's members: those with columns (group_view)
    for (int i = 0; i < count; ++i)
        if (members[i].plan->cols > 0) cols[n++] = members[i].plan->cols;
    const int rt = tcsc::decode_row_tiles(M), cus = members[0].plan->num_cus;
    const int t = rt > 1 ? tcsc::decode_group_rows_tiles_per_wg(M, cols, n, cus)
                         : tcsc::decode_group_tiles_per_wg(M, cols, n, cus);
    *row_tiles = rt;
    *col_tiles = t;
    *workgroups = tcsc::decode_group_wgs(cols, n, t);
    return TCSC_OK;
}

int tcsc_gpu_workspace_bound_i8(int M, int K, int N, size_t* i8_bytes, size_t* f32_bytes) {
    if (M < 0 || K < 1 || N < 0) {
        set_error("tcsc_gpu_workspace_bound_i8: bad arguments (M=%d K=%d N=%d)", M, K, N);
        return TCSC_E_ARG;
    }
    if (i8_bytes) *i8_bytes = mfma_ws(kI8, M, K, N).bytes;
    if (f32_bytes) *f32_bytes = mfma_ws(kF32, M, K, N).bytes;
    return TCSC_OK;
}

static int ensure_workspace(const tcsc_gpu_plan* p, int M) {
    if (p && M > 0 && p->cols > 0 && p->ws_bytes < wanted_workspace(p, M))
        return tcsc_gpu_plan_reserve(const_cast<tcsc_gpu_plan*>(p), M);
    return TCSC_OK;
}

int tcsc_gpu_prepare_x(const tcsc_gpu_plan* p, const float* dX, int M, void* stream) {
    if (refuse_packed(p, "tcsc_gpu_prepare_x")) return TCSC_E_ARG;
    int rc = ensure_workspace(p, M);
    if (rc != TCSC_OK) return rc;
    if (p) const_cast<tcsc_gpu_plan*>(p)->staged_M = -1;
    rc = sgemm_ws(p, make_call(dX, kF32, nullptr, nullptr, YOut{}, M, 0, 0, 0.f, stream), p ? p->ws : nullptr,
                  p ? p->ws_bytes : 0, 1, RoutePins(), nullptr);
    if (rc == TCSC_OK && p) const_cast<tcsc_gpu_plan*>(p)->staged_M = M;
    return rc;
}

int tcsc_gpu_sgemm_prepared(const tcsc_gpu_plan* p, const float* dB, float* dY, int M, int ldy, int variant, float a,
                            void* stream) {
    if (refuse_packed(p, "tcsc_gpu_sgemm_prepared")) return TCSC_E_ARG;
    const int rc = ensure_workspace(p, M);  // a reallocation drops the staged X
    if (rc != TCSC_OK) return rc;
    // the gather reads X^T with the pitch of the M it was staged for
    if (p && M > 0 && p->cols > 0 && p->rows > 0 && p->staged_M != M) {
        set_error("tcsc_gpu_sgemm_prepared: M=%d but %s (call tcsc_gpu_prepare_x with this M first)", M,
                  p->staged_M < 0 ? "no X is staged" : "the staged X has another M");
        return TCSC_E_ARG;
    }
    return sgemm_ws(p, make_call(nullptr, kF32, nullptr, dB, YOut{dY, kYF32, nullptr}, M, ldy, variant, a, stream),
                    p ? p->ws : nullptr, p ? p->ws_bytes : 0, 2, RoutePins(), nullptr);
}

// The two calls (counts, then fill) share the tile offsets: the first call
// keeps them per device, keyed by (matrix, shape, col_start arrays), and the
// very next call on the same key fills from them instead of counting again
// (cfg 4: two reads of the 1-GiB matrix in all instead of three).  Any other
// call in between drops the kept counts (the next call counts afresh), and
// include/tcsc_gpu.h requires the matrix to stay unchanged between the two
// calls of a pair.  The fill writes at most the counted entries, so index
// arrays sized from the first call are never overrun even if it did change.
struct DenseBuildScratch {
    const float* key = nullptr;
    const int* key_csp = nullptr;
    const int* key_csn = nullptr;
    int rows = -1, cols = -1;
    bool counted = false;
    DevBuf cp, cn, totp, totn, tmp;
    size_t tile_cap = 0, col_cap = 0, tmp_cap = 0;
};
std::mutex g_build_mu;
std::vector<DenseBuildScratch> g_build;

int tcsc_gpu_from_dense(const float* d_dense, int rows, int cols, int* d_csp, int* d_csn, int* d_rip, int* d_rin,
                        int* n_pos, int* n_neg, void* stream) {
    if (!d_csp || !d_csn || !n_pos || !n_neg || rows < 0 || cols < 0 || (!d_dense && rows * (long long)cols)) {
        set_error("tcsc_gpu_from_dense: bad arguments");
        return TCSC_E_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_build_mu);
    if ((int)g_build.size() <= dev) g_build.resize(dev + 1);
    DenseBuildScratch& sc = g_build[dev];
    const int tr = tcsc::dense_tile_rows(rows), nt = rows > 0 ? (rows + tr - 1) / tr : 0;
    const size_t tile_b = std::max<size_t>(1, (size_t)nt * cols) * sizeof(int);
    const size_t col_b = (size_t)(cols + 1) * sizeof(int);
    const bool reuse = sc.counted && sc.key == d_dense && sc.key_csp == d_csp && sc.key_csn == d_csn &&
                       sc.rows == rows && sc.cols == cols && d_rip && d_rin;
    if (!reuse) {
        auto grow = [](DevBuf& b, size_t& cap, size_t want) -> hipError_t {
            if (cap >= want && b.p) return hipSuccess;
            if (b.p) (void)hipFree(b.p);
            b.p = nullptr;
            cap = 0;
            const hipError_t e = b.alloc(want);
            if (e == hipSuccess) cap = want;
            return e;
        };
        size_t tb = 0;
        HIP_TRY(tcsc::plan_scan_tmp_bytes(cols + 1, &tb));
        size_t c1 = sc.tile_cap, c2 = sc.col_cap;
        HIP_TRY(grow(sc.cp, sc.tile_cap, tile_b));
        HIP_TRY(grow(sc.cn, c1, tile_b));
        HIP_TRY(grow(sc.totp, sc.col_cap, col_b));
        HIP_TRY(grow(sc.totn, c2, col_b));
        HIP_TRY(grow(sc.tmp, sc.tmp_cap, tb));
        sc.counted = false;
        HIP_TRY(tcsc::dense_to_tcsc_counts(d_dense, rows, cols, sc.cp.as<int>(), sc.cn.as<int>(), sc.totp.as<int>(),
                                           sc.totn.as<int>(), st));
        sc.key = d_dense;
        sc.key_csp = d_csp;
        sc.key_csn = d_csn;
        sc.rows = rows;
        sc.cols = cols;
        sc.counted = true;
    }
    size_t tb = sc.tmp_cap;
    HIP_TRY(tcsc::exclusive_scan_i32(sc.totp.as<int>(), d_csp, cols + 1, sc.tmp.p, tb, st));
    HIP_TRY(tcsc::exclusive_scan_i32(sc.totn.as<int>(), d_csn, cols + 1, sc.tmp.p, tb, st));
    int tot[2];
    HIP_TRY(hipMemcpyAsync(&tot[0], d_csp + cols, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&tot[1], d_csn + cols, sizeof(int), hipMemcpyDeviceToHost, st));
    if (d_rip && d_rin && cols > 0 && rows > 0)
        HIP_TRY(tcsc::dense_to_tcsc_fill(d_dense, rows, cols, d_csp, d_csn, sc.cp.as<int>(), sc.cn.as<int>(), d_rip,
                                         d_rin, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (d_rip && d_rin) sc.counted = false;  // a fill ends the pair
    *n_pos = tot[0];
    *n_neg = tot[1];
    return TCSC_OK;
}

// Dense baseline: the reference's gemm_basic
// (dense/dense.c:64-77, y = sum_k X[m,k] W[k,n], then + B[n]) on the device:
// rocBLAS fp32 SGEMM with the dense ternary W, then the bias (+PReLU)
// epilogue kernel.  Row-major Y = X W is the column-major product
// Y^T (N x M, ld ldy) = W^T (N x K, ld N) * X^T (K x M, ld K).
int tcsc_gpu_dense_sgemm(const float* dX, const float* dW, const float* dB, float* dY, int M, int N, int K,
                         int ldy, int variant, float a, void* stream) {
    if (M < 0 || N < 0 || K < 0 || ldy < N || !valid_variant(variant) ||
        ((long long)M * N > 0 && (!dX || !dW || !dB || !dY))) {
        set_error("tcsc_gpu_dense_sgemm: bad arguments (M=%d N=%d K=%d ldy=%d variant=%d)", M, N, K, ldy, variant);
        return TCSC_E_ARG;
    }
    if (M == 0 || N == 0) return TCSC_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    rocblas_handle h = rocblas_for_device(dev);
    if (!h) {
        set_error("tcsc_gpu_dense_sgemm: rocblas_create_handle failed");
        return TCSC_E_HIP;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (rocblas_set_stream(h, st) != rocblas_status_success) {
        set_error("tcsc_gpu_dense_sgemm: rocblas_set_stream failed");
        return TCSC_E_HIP;
    }
    const float one = 1.0f, zero = 0.0f;
    if (K == 0) {
        HIP_TRY(hipMemset2DAsync(dY, (size_t)ldy * sizeof(float), 0, (size_t)N * sizeof(float), M, st));
    } else {
        const rocblas_status rs = rocblas_sgemm(h, rocblas_operation_none, rocblas_operation_none, N, M, K, &one, dW,
                                                N, dX, K, &zero, dY, ldy);
        if (rs != rocblas_status_success) {
            set_error("tcsc_gpu_dense_sgemm: rocblas_sgemm failed (%s)", rocblas_status_to_string(rs));
            return TCSC_E_HIP;
        }
    }
    HIP_TRY(tcsc::launch_bias_act(dY, M, N, ldy, dB, is_prelu(variant), a, st));
    return TCSC_OK;
}

// ---- backward pass -------------------------------------------

// The arguments every transpose entry point shares, checked before any HIP call.
static int transpose_args_ok(const char* who, int rows, int cols, const int* d_csp, const int* d_csn, int col_begin,
                             int col_end) {
    if (rows < 0 || cols < 0 || col_begin < 0 || col_end > cols || col_begin > col_end ||
        (col_end > col_begin && (!d_csp || !d_csn))) {
        set_error("%s: bad arguments (rows=%d cols=%d range [%d, %d)%s)", who, rows, cols, col_begin, col_end,
                  (!d_csp || !d_csn) ? ", NULL col_start" : "");
        return TCSC_E_ARG;
    }
    return TCSC_OK;
}

// ends = {csp[col_begin], csp[col_end], csn[col_begin], csn[col_end]} (zeros for an empty range)
static int read_range_ends(const int* d_csp, const int* d_csn, int col_begin, int col_end, int ends[4],
                           hipStream_t st) {
    ends[0] = ends[1] = ends[2] = ends[3] = 0;
    if (col_end <= col_begin) return TCSC_OK;
    HIP_TRY(hipMemcpyAsync(&ends[0], d_csp + col_begin, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[1], d_csp + col_end, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[2], d_csn + col_begin, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ends[3], d_csn + col_end, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TCSC_OK;
}

// The transpose proper, `ends` already read.  Validates the input range
// (check_index_device: bit 0 is an error, bit 1 -- a column out of order -- is
// not: the output does not depend on the order inside an input column), then
// per sign: histogram, scan, scatter, per-column sort.  Synchronises st.
static int transpose_index_impl(const char* who, int rows, const int* d_csp, const int* d_csn, const int* d_rip,
                                const int* d_rin, int col_begin, int col_end, const int ends[4], int* d_t_csp,
                                int* d_t_csn, int* d_t_rip, int* d_t_rin, hipStream_t st) {
    const int nc = col_end - col_begin;
    const int np = ends[1] - ends[0], nn = ends[3] - ends[2];
    if (nc > 0 && (np < 0 || nn < 0 || ends[0] < 0 || ends[2] < 0)) {
        set_error("%s: col_start decreases over the column range", who);
        return TCSC_E_ARG;
    }
    if ((np > 0 && (!d_rip || !d_t_rip)) || (nn > 0 && (!d_rin || !d_t_rin))) {
        set_error("%s: NULL row index array (n_pos=%d n_neg=%d in the range)", who, np, nn);
        return TCSC_E_ARG;
    }
    if (nc == 0 || rows == 0 || np + (long long)nn == 0) {
        // nothing to move: the offsets are still written, all zero
        if (nc > 0 && rows == 0 && np + (long long)nn > 0) {
            set_error("%s: entries in a matrix of 0 rows", who);
            return TCSC_E_ARG;
        }
        HIP_TRY(hipMemsetAsync(d_t_csp, 0, (size_t)(rows + 1) * sizeof(int), st));
        HIP_TRY(hipMemsetAsync(d_t_csn, 0, (size_t)(rows + 1) * sizeof(int), st));
        HIP_TRY(hipStreamSynchronize(st));
        return TCSC_OK;
    }
    DevBuf flag, cnt, cursor, unsorted, tmp;
    HIP_TRY(flag.alloc(sizeof(int)));
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    HIP_TRY(tcsc::check_index_device(d_csp, d_rip, col_begin, nc, rows, ends[1], flag.as<int>(), st));
    HIP_TRY(tcsc::check_index_device(d_csn, d_rin, col_begin, nc, rows, ends[3], flag.as<int>(), st));
    int hflag = 0;
    HIP_TRY(hipMemcpyAsync(&hflag, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hflag & 1) {
        set_error("%s: a col_start range or a row index outside [0, %d)", who, rows);
        return TCSC_E_ARG;
    }
    const int nmax = std::max(np, nn);
    size_t tb_scan = 0, tb_sort = 0;
    HIP_TRY(tcsc::plan_scan_tmp_bytes((long long)rows + 1, &tb_scan));
    HIP_TRY(tcsc::sort_columns_tmp_bytes(nmax, rows, &tb_sort));
    const size_t tb = std::max(tb_scan, tb_sort);
    HIP_TRY(cnt.alloc((size_t)(rows + 1) * sizeof(int)));
    HIP_TRY(cursor.alloc((size_t)(rows + 1) * sizeof(int)));
    HIP_TRY(unsorted.alloc((size_t)nmax * sizeof(int)));
    HIP_TRY(tmp.alloc(tb));
    HIP_TRY(tcsc::transpose_sign(d_csp, d_rip, col_begin, nc, rows, ends[0], np, cnt.as<int>(), cursor.as<int>(),
                                 unsorted.as<int>(), tmp.p, tb, d_t_csp, d_t_rip, st));
    HIP_TRY(tcsc::transpose_sign(d_csn, d_rin, col_begin, nc, rows, ends[2], nn, cnt.as<int>(), cursor.as<int>(),
                                 unsorted.as<int>(), tmp.p, tb, d_t_csn, d_t_rin, st));
    HIP_TRY(hipStreamSynchronize(st));  // the scratch is freed on return
    return TCSC_OK;
}

int tcsc_gpu_transpose_index(int rows, int cols, const int* d_csp, const int* d_csn, const int* d_rip,
                             const int* d_rin, int col_begin, int col_end, int* d_t_csp, int* d_t_csn, int* d_t_rip,
                             int* d_t_rin, void* stream) {
    const int rc = transpose_args_ok("tcsc_gpu_transpose_index", rows, cols, d_csp, d_csn, col_begin, col_end);
    if (rc != TCSC_OK) return rc;
    if (!d_t_csp || !d_t_csn) {
        set_error("tcsc_gpu_transpose_index: NULL output col_start array");
        return TCSC_E_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    int ends[4];
    const int re = read_range_ends(d_csp, d_csn, col_begin, col_end, ends, st);
    if (re != TCSC_OK) return re;
    return transpose_index_impl("tcsc_gpu_transpose_index", rows, d_csp, d_csn, d_rip, d_rin, col_begin, col_end, ends,
                                d_t_csp, d_t_csn, d_t_rip, d_t_rin, st);
}

// The plan of W[:, col_begin:col_end)^T from device arrays of W (the current
// device is `device`): transposed index arrays in scratch, an ordinary plan
// built from them, and the plan's zero bias.
static int plan_create_transposed_impl(const char* who, int rows, const int* d_csp, const int* d_csn,
                                       const int* d_rip, const int* d_rin, int col_begin, int col_end, int device,
                                       hipStream_t st, tcsc_gpu_plan** out) {
    int ends[4];
    int rc = read_range_ends(d_csp, d_csn, col_begin, col_end, ends, st);
    if (rc != TCSC_OK) return rc;
    const int nc = col_end - col_begin;
    const int np = std::max(ends[1] - ends[0], 0), nn = std::max(ends[3] - ends[2], 0);
    DevBuf tcsp, tcsn, trip, trin;
    HIP_TRY(tcsp.alloc((size_t)(rows + 1) * sizeof(int)));
    HIP_TRY(tcsn.alloc((size_t)(rows + 1) * sizeof(int)));
    HIP_TRY(trip.alloc((size_t)np * sizeof(int)));
    HIP_TRY(trin.alloc((size_t)nn * sizeof(int)));
    rc = transpose_index_impl(who, rows, d_csp, d_csn, d_rip, d_rin, col_begin, col_end, ends, tcsp.as<int>(),
                              tcsn.as<int>(), trip.as<int>(), trin.as<int>(), st);
    if (rc != TCSC_OK) return rc;
    // W^T of the range: nc rows, `rows` columns, every column in order
    rc = build_plan_ordered(nc, 0, rows, np, nn, tcsp.as<int>(), tcsn.as<int>(), trip.as<int>(), trin.as<int>(),
                            device, st, current_order(), out);
    if (rc != TCSC_OK) return rc;
    std::unique_ptr<tcsc_gpu_plan, PlanDeleter> plan(*out);
    *out = nullptr;
    const size_t bb = std::max<size_t>((size_t)rows * sizeof(float), 4);
    HIP_TRY(hipMalloc(&plan->tbias, bb));
    plan->tbias_bytes = bb;
    HIP_TRY(hipMemsetAsync(plan->tbias, 0, bb, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = plan.release();
    return TCSC_OK;
}

int tcsc_gpu_plan_create_transposed_device(int rows, int cols, const int* d_csp, const int* d_csn, const int* d_rip,
                                           const int* d_rin, int col_begin, int col_end, int device, void* stream,
                                           tcsc_gpu_plan** out) {
    const char* who = "tcsc_gpu_plan_create_transposed_device";
    const int rc = transpose_args_ok(who, rows, cols, d_csp, d_csn, col_begin, col_end);
    if (rc != TCSC_OK) return rc;
    if (!out) {
        set_error("%s: NULL out", who);
        return TCSC_E_ARG;
    }
    *out = nullptr;
    DeviceGuard dg(device);
    if (!dg.ok()) {
        set_error("%s: cannot select device %d", who, device);
        return TCSC_E_NODEV;
    }
    return plan_create_transposed_impl(who, rows, d_csp, d_csn, d_rip, d_rin, col_begin, col_end, device,
                                       static_cast<hipStream_t>(stream), out);
}

int tcsc_gpu_plan_create_transposed(const tcsc_t* W, int col_begin, int col_end, int device, void* stream,
                                    tcsc_gpu_plan** out) {
    const char* who = "tcsc_gpu_plan_create_transposed";
    if (!W || !out || col_begin < 0 || col_end > W->cols || col_begin > col_end || W->rows < 0) {
        set_error("%s: bad arguments", who);
        return TCSC_E_ARG;
    }
    *out = nullptr;
    const int nc = col_end - col_begin;
    // the host check of tcsc_gpu_plan_create; the sorted copies are not needed
    // (the transpose does not depend on the order inside an input column)
    std::vector<int> unused;
    int rc = check_index_host(W->col_start_pos, W->row_index_pos, col_begin, col_end, W->rows, W->n_elem_pos, "pos",
                              unused);
    if (rc == TCSC_OK)
        rc = check_index_host(W->col_start_neg, W->row_index_neg, col_begin, col_end, W->rows, W->n_elem_neg, "neg",
                              unused);
    if (rc != TCSC_OK) return rc;
    unused = std::vector<int>();
    DeviceGuard dg(device);
    if (!dg.ok()) {
        set_error("%s: cannot select device %d", who, device);
        return TCSC_E_NODEV;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int p0 = W->col_start_pos[col_begin], p1 = W->col_start_pos[col_end];
    const int q0 = W->col_start_neg[col_begin], q1 = W->col_start_neg[col_end];
    // column slice, rebased to 0 (as tcsc_gpu_plan_create uploads it)
    std::vector<int> csp(nc + 1), csn(nc + 1);
    for (int j = 0; j <= nc; ++j) {
        csp[j] = W->col_start_pos[col_begin + j] - p0;
        csn[j] = W->col_start_neg[col_begin + j] - q0;
    }
    DevBuf dcsp, dcsn, drip, drin;
    HIP_TRY(dcsp.alloc((nc + 1) * sizeof(int)));
    HIP_TRY(dcsn.alloc((nc + 1) * sizeof(int)));
    HIP_TRY(drip.alloc((size_t)(p1 - p0) * sizeof(int)));
    HIP_TRY(drin.alloc((size_t)(q1 - q0) * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(dcsp.p, csp.data(), (nc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dcsn.p, csn.data(), (nc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (p1 > p0)
        HIP_TRY(hipMemcpyAsync(drip.p, W->row_index_pos + p0, (size_t)(p1 - p0) * sizeof(int), hipMemcpyHostToDevice,
                               st));
    if (q1 > q0)
        HIP_TRY(hipMemcpyAsync(drin.p, W->row_index_neg + q0, (size_t)(q1 - q0) * sizeof(int), hipMemcpyHostToDevice,
                               st));
    HIP_TRY(hipStreamSynchronize(st));  // csp / csn are pageable host vectors
    return plan_create_transposed_impl(who, W->rows, dcsp.as<int>(), dcsn.as<int>(), drip.as<int>(), drin.as<int>(), 0,
                                       nc, device, st, out);
}

int tcsc_gpu_sgemm_t(const tcsc_gpu_plan* tplan, const float* dG, float* dDX, int M, int ldx, void* stream) {
    if (!tplan) {
        set_error("tcsc_gpu_sgemm_t: NULL plan");
        return TCSC_E_ARG;
    }
    if (refuse_packed(tplan, "tcsc_gpu_sgemm_t")) return TCSC_E_ARG;
    if (!tplan->tbias) {
        set_error("tcsc_gpu_sgemm_t: not a transposed plan (tcsc_gpu_plan_create_transposed*)");
        return TCSC_E_ARG;
    }
    if (M < 0 || ldx < tplan->cols || ((long long)M * tplan->cols > 0 && (!dDX || (!dG && tplan->rows > 0)))) {
        set_error("tcsc_gpu_sgemm_t: bad arguments (M=%d ldx=%d < K=%d, or a NULL device pointer)", M, ldx,
                  tplan->cols);
        return TCSC_E_ARG;
    }
    return tcsc_gpu_sgemm(tplan, dG, tplan->tbias, dDX, M, ldx, TCSC_VARIANT_SPARSE_GEMM, 0.0f, stream);
}

int tcsc_gpu_prelu_backward(const float* dG, int ldg, const float* dY, int ldy, float a, float* dDZ, int lddz,
                            float* dDB, int M, int N, void* stream) {
    if (M < 0 || N < 0 || ldg < N || (dY && ldy < N) || (dDZ && lddz < N)) {
        set_error("tcsc_gpu_prelu_backward: bad arguments (M=%d N=%d ldg=%d ldy=%d lddz=%d)", M, N, ldg, ldy, lddz);
        return TCSC_E_ARG;
    }
    if (!dG && (long long)M * N > 0) {
        set_error("tcsc_gpu_prelu_backward: NULL G");
        return TCSC_E_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (N == 0) return TCSC_OK;
    if (M == 0) {  // the sum over no rows
        if (dDB) HIP_TRY(hipMemsetAsync(dDB, 0, (size_t)N * sizeof(float), st));
        return TCSC_OK;
    }
    if (!dDZ && !dDB) return TCSC_OK;
    HIP_TRY(tcsc::launch_prelu_bwd(dG, ldg, dY, ldy, a, dDZ, lddz, dDB, M, N, st));
    return TCSC_OK;
}

}  // extern "C"

