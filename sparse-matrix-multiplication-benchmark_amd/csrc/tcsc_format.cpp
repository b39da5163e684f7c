// tcsc_format.cpp -- tcsc_from_dense and the harness's dense helpers.
//
// tcsc_from_dense keeps the reference's contract bit-for-bit
// (sparse/tcsc.c:6-66): only values comparing equal to +1.0f / -1.0f are
// stored, rows ascend inside every column, col_start_* have cols+1 entries,
// NULL is returned on allocation failure.  The reference's fill pass walks W
// column by column with stride `cols` (tcsc.c:48-60, 6-7 s at K=N=16384);
// this builder reads W row-major twice (count, then fill through per-column
// cursors), which visits each column's rows in ascending order too, so the
// output is identical.
//
// Large inputs go to the device builder (tcsc_gpu_from_dense, same result)
// when a GPU is present; TCSC_BUILDER=host|gpu forces one side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <system_error>
#include <thread>
#include <vector>
#include <sched.h>

#include "../../include/dense/dense.h"
#include "../../include/sparse/tcsc.h"
#include "../../include/tcsc_gpu.h"
#include "tcsc_internal.h"

namespace {

// ---- the 2-bit image on the host (tcsc_gpu_w2_*_host) ---------
// The layout of tcsc_internal.h, byte-wise (the image is little-endian dwords):
// weight (k, col) lives in byte w2_byte(...) at bit 2 (j >> 2), j = k % 16.
inline size_t w2_byte(int k, int col, int nkb) {
    const int kk = k % tcsc::kW2Blk, i = kk / 64, q = (kk % 64) / 16, j = kk % 16;
    const size_t tile = (size_t)(col / tcsc::kW2Cols) * nkb + k / tcsc::kW2Blk;
    return ((tile * 64 + 16 * q + col % tcsc::kW2Cols) * 4 + i) * 4 + (j & 3);
}
inline int w2_shift(int k) { return 2 * ((k % 16) >> 2); }

bool w2_host_fail(const char* who, const char* what) {  // records the message; false, for `return`
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s: %s", who, what);
    tcsc::set_error_msg(buf);
    return false;
}

bool w2_host_args_ok(const char* who, const void* image, size_t bytes, int rows, int cols) {
    if (!image) return w2_host_fail(who, "NULL image");
    if (rows < 1 || rows >= tcsc::kDecodeMaxK) return w2_host_fail(who, "an image needs 1 <= K < 2^22");
    if (cols < 1) return w2_host_fail(who, "no columns (cols < 1, or an empty column range)");
    if (bytes != tcsc::w2_image_bytes(rows, cols))
        return w2_host_fail(who, "bytes is not tcsc_gpu_w2_image_bytes(rows, cols)");
    return true;
}

// one sign's lists of columns [c0, c1): ranges inside [0, n) that do not run backwards, rows inside [0, K)
bool w2_host_index_ok(const char* who, const int* cs, const int* ri, int c0, int c1, int n, int K) {
    if (!cs || (n > 0 && !ri)) return w2_host_fail(who, "NULL index array");
    for (int j = c0; j < c1; ++j)
        if (cs[j] < 0 || cs[j + 1] < cs[j] || cs[j + 1] > n) return w2_host_fail(who, "a col_start that is no range");
    for (int e = cs[c0]; e < cs[c1]; ++e)
        if (ri[e] < 0 || ri[e] >= K) return w2_host_fail(who, "a row index outside [0, K)");
    return true;
}

tcsc_t* alloc_tcsc(int rows, int cols, int n_pos, int n_neg) {
    tcsc_t* t = static_cast<tcsc_t*>(std::malloc(sizeof(tcsc_t)));
    if (!t) return nullptr;
    t->rows = rows;
    t->cols = cols;
    t->n_elem_pos = n_pos;
    t->n_elem_neg = n_neg;
    t->col_start_pos = static_cast<int*>(std::malloc(((size_t)cols + 1) * sizeof(int)));
    t->col_start_neg = static_cast<int*>(std::malloc(((size_t)cols + 1) * sizeof(int)));
    // malloc(0) is allowed to return NULL; keep a valid pointer instead
    t->row_index_pos = static_cast<int*>(std::malloc((size_t)(n_pos > 0 ? n_pos : 1) * sizeof(int)));
    t->row_index_neg = static_cast<int*>(std::malloc((size_t)(n_neg > 0 ? n_neg : 1) * sizeof(int)));
    if (!t->col_start_pos || !t->col_start_neg || !t->row_index_pos || !t->row_index_neg) {
        std::free(t->col_start_pos);
        std::free(t->col_start_neg);
        std::free(t->row_index_pos);
        std::free(t->row_index_neg);
        std::free(t);
        return nullptr;
    }
    return t;
}

tcsc_t* from_dense_host(const float* D, int rows, int cols) {
    std::vector<int> cp((size_t)cols + 1, 0), cn((size_t)cols + 1, 0);
    for (int i = 0; i < rows; ++i) {
        const float* r = D + (size_t)i * cols;
        for (int j = 0; j < cols; ++j) {
            const float v = r[j];
            cp[j] += (v == 1.0f);
            cn[j] += (v == -1.0f);
        }
    }
    long long P = 0, Q = 0;
    for (int j = 0; j < cols; ++j) {
        P += cp[j];
        Q += cn[j];
    }
    if (P > 0x7fffffffLL || Q > 0x7fffffffLL) return nullptr;
    tcsc_t* t = alloc_tcsc(rows, cols, (int)P, (int)Q);
    if (!t) return nullptr;
    int p = 0, q = 0;
    for (int j = 0; j < cols; ++j) {
        t->col_start_pos[j] = p;
        t->col_start_neg[j] = q;
        p += cp[j];
        q += cn[j];
    }
    t->col_start_pos[cols] = p;
    t->col_start_neg[cols] = q;
    // cursors
    for (int j = 0; j < cols; ++j) {
        cp[j] = t->col_start_pos[j];
        cn[j] = t->col_start_neg[j];
    }
    for (int i = 0; i < rows; ++i) {
        const float* r = D + (size_t)i * cols;
        for (int j = 0; j < cols; ++j) {
            const float v = r[j];
            if (v == 1.0f)
                t->row_index_pos[cp[j]++] = i;
            else if (v == -1.0f)
                t->row_index_neg[cn[j]++] = i;
        }
    }
    return t;
}

tcsc_t* from_dense_gpu(const float* D, int rows, int cols) {
    const size_t bytes = (size_t)rows * cols * sizeof(float);
    float* dD = nullptr;
    int *dcsp = nullptr, *dcsn = nullptr, *drip = nullptr, *drin = nullptr;
    tcsc_t* t = nullptr;
    int np = 0, nn = 0;
    hipStream_t st = nullptr;
    bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(&dD, bytes ? bytes : 4) == hipSuccess &&
              hipMalloc(&dcsp, ((size_t)cols + 1) * sizeof(int)) == hipSuccess &&
              hipMalloc(&dcsn, ((size_t)cols + 1) * sizeof(int)) == hipSuccess &&
              hipMemcpyAsync(dD, D, bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
              tcsc_gpu_from_dense(dD, rows, cols, dcsp, dcsn, nullptr, nullptr, &np, &nn, st) == TCSC_OK &&
              hipMalloc(&drip, (size_t)(np > 0 ? np : 1) * sizeof(int)) == hipSuccess &&
              hipMalloc(&drin, (size_t)(nn > 0 ? nn : 1) * sizeof(int)) == hipSuccess &&
              tcsc_gpu_from_dense(dD, rows, cols, dcsp, dcsn, drip, drin, &np, &nn, st) == TCSC_OK &&
              (t = alloc_tcsc(rows, cols, np, nn)) != nullptr &&
              hipMemcpyAsync(t->col_start_pos, dcsp, ((size_t)cols + 1) * sizeof(int), hipMemcpyDeviceToHost,
                             st) == hipSuccess &&
              hipMemcpyAsync(t->col_start_neg, dcsn, ((size_t)cols + 1) * sizeof(int), hipMemcpyDeviceToHost,
                             st) == hipSuccess &&
              hipMemcpyAsync(t->row_index_pos, drip, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, st) ==
                  hipSuccess &&
              hipMemcpyAsync(t->row_index_neg, drin, (size_t)nn * sizeof(int), hipMemcpyDeviceToHost, st) ==
                  hipSuccess &&
              hipStreamSynchronize(st) == hipSuccess;
    if (dD) (void)hipFree(dD);
    if (dcsp) (void)hipFree(dcsp);
    if (dcsn) (void)hipFree(dcsn);
    if (drip) (void)hipFree(drip);
    if (drin) (void)hipFree(drin);
    if (st) (void)hipStreamDestroy(st);
    if (!ok) {
        (void)hipGetLastError();
        if (t) tcsc_free(t);
        return nullptr;
    }
    return t;
}

// --- SplitMix64 generators (reproducible replacement for the reference's
// std::random_device-seeded mt19937, dense/utils.h:11,57) ---------------
uint64_t g_seed = 0x7C5C0000ull;

inline uint64_t splitmix64(uint64_t* s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

float* aligned_floats(size_t n) {
    void* p = nullptr;
    if (posix_memalign(&p, 32, (n ? n : 1) * sizeof(float)) != 0) {
        std::perror("posix_memalign failed");
        std::exit(EXIT_FAILURE);
    }
    return static_cast<float*>(p);
}

}  // namespace

extern "C" {

tcsc_t* tcsc_from_dense(dense_t dense, int rows, int cols) {
    if (rows < 0 || cols < 0 || (!dense && (long long)rows * cols > 0)) return nullptr;
    const char* mode = std::getenv("TCSC_BUILDER");
    const long long n = (long long)rows * cols;
    bool gpu = n >= (1LL << 24);  // ~64 MB and up: PCIe + device beats two host passes
    if (mode && std::strcmp(mode, "host") == 0) gpu = false;
    if (mode && std::strcmp(mode, "gpu") == 0) gpu = true;
    static const bool trace = std::getenv("TCSC_HOST_PATHS") != nullptr;
    if (gpu && tcsc_gpu_device_count() > 0) {
        tcsc_t* t = from_dense_gpu(dense, rows, cols);
        if (trace) std::fprintf(stderr, "[tcsc_amd] tcsc_from_dense %dx%d: device builder%s\n", rows, cols, t ? "" : " failed");
        if (t || (mode && std::strcmp(mode, "gpu") == 0)) return t;
    }
    if (trace) std::fprintf(stderr, "[tcsc_amd] tcsc_from_dense %dx%d: host builder\n", rows, cols);
    return from_dense_host(dense, rows, cols);
}

// The image of W[:, col_begin:col_end) in host code: k_w2_from_tcsc's semantics
// and bytes.  Per column the weights are summed into a K-long scratch (a +1 and
// a -1 at one position cancel, the order inside a column does not matter), the
// touched positions are written, and the scratch is cleared again.
int tcsc_gpu_w2_from_tcsc_host(const tcsc_t* W, int col_begin, int col_end, void* image, size_t bytes) {
    const char* who = "tcsc_gpu_w2_from_tcsc_host";
    if (!W) return w2_host_fail(who, "NULL W"), TCSC_E_ARG;
    if (col_begin < 0 || col_end > W->cols || col_begin > col_end)
        return w2_host_fail(who, "a column range outside W"), TCSC_E_ARG;
    const int K = W->rows, nc = col_end - col_begin;
    if (!w2_host_args_ok(who, image, bytes, K, nc)) return TCSC_E_ARG;
    if (!w2_host_index_ok(who, W->col_start_pos, W->row_index_pos, col_begin, col_end, W->n_elem_pos, K) ||
        !w2_host_index_ok(who, W->col_start_neg, W->row_index_neg, col_begin, col_end, W->n_elem_neg, K))
        return TCSC_E_ARG;
    uint8_t* img = static_cast<uint8_t*>(image);
    std::memset(img, 0x55, bytes);  // code 1 everywhere: weight 0, and the padding
    const int nkb = tcsc::w2_kblocks(K);
    std::vector<int> w((size_t)K, 0);
    const int* cs[2] = {W->col_start_pos, W->col_start_neg};
    const int* ri[2] = {W->row_index_pos, W->row_index_neg};
    for (int c = 0; c < nc; ++c) {
        const int j = col_begin + c;
        bool ok = true;
        for (int s = 0; s < 2; ++s)
            for (int e = cs[s][j]; e < cs[s][j + 1]; ++e) w[ri[s][e]] += s ? -1 : 1;  // fewer than 2^31 entries a sign
        for (int s = 0; s < 2; ++s)
            for (int e = cs[s][j]; e < cs[s][j + 1]; ++e) {
                const int k = ri[s][e], v = w[k];
                if (v < -1 || v > 1) ok = false;
                uint8_t& b = img[w2_byte(k, c, nkb)];
                b = (uint8_t)((b & ~(3u << w2_shift(k))) | ((unsigned)((v + 1) & 3) << w2_shift(k)));
            }
        for (int s = 0; s < 2; ++s)
            for (int e = cs[s][j]; e < cs[s][j + 1]; ++e) w[ri[s][e]] = 0;
        if (!ok)
            return w2_host_fail(who, "W is not ternary: a position's summed weight is outside {-1, 0, +1} "
                                     "(a duplicated index)"), TCSC_E_ARG;
    }
    return TCSC_OK;
}

// The image back to a tcsc_t: tcsc_gpu_w2_to_tcsc's validation and arrays.  Two
// walks over the image in tile order; inside a column tile the k blocks, steps,
// quarters and j ascend, so every column's cursor sees its rows ascending.
tcsc_t* tcsc_gpu_w2_to_tcsc_host(const void* image, size_t bytes, int rows, int cols) {
    const char* who = "tcsc_gpu_w2_to_tcsc_host";
    if (!w2_host_args_ok(who, image, bytes, rows, cols)) return nullptr;
    const uint8_t* img = static_cast<const uint8_t*>(image);
    const int nkb = tcsc::w2_kblocks(rows), nt = tcsc::w2_col_tiles(cols);
    std::vector<long long> cp((size_t)cols + 1, 0), cn((size_t)cols + 1, 0);
    tcsc_t* t = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        for (int ct = 0; ct < nt; ++ct)
            for (int kb = 0; kb < nkb; ++kb)
                for (int i = 0; i < 4; ++i)
                    for (int q = 0; q < 4; ++q)
                        for (int c = 0; c < tcsc::kW2Cols; ++c) {
                            const int col = tcsc::kW2Cols * ct + c, k0 = tcsc::kW2Blk * kb + 64 * i + 16 * q;
                            const uint8_t* d = img + ((((size_t)ct * nkb + kb) * 64 + 16 * q + c) * 4 + i) * 4;
                            for (int j = 0; j < 16; ++j) {
                                const int code = d[j & 3] >> (2 * (j >> 2)) & 3, k = k0 + j;
                                if (pass) {
                                    if (code == 2) t->row_index_pos[cp[col]++] = k;
                                    if (code == 0) t->row_index_neg[cn[col]++] = k;
                                    continue;
                                }
                                if (code == 3) return w2_host_fail(who, "invalid image: a code 3 (no ternary weight)"), nullptr;
                                if (col >= cols || k >= rows) {
                                    if (code != 1)
                                        return w2_host_fail(who, "invalid image: padding (k >= rows or column >= cols) "
                                                                 "holds a code other than 1"), nullptr;
                                    continue;
                                }
                                cp[col] += code == 2;
                                cn[col] += code == 0;
                            }
                        }
        if (pass) break;
        long long p = 0, n = 0;  // counts -> offsets, which the fill pass uses as cursors
        for (int j = 0; j <= cols; ++j) {
            const long long a = cp[j], b = cn[j];
            cp[j] = p;
            cn[j] = n;
            p += a;
            n += b;
        }
        if (p > 0x7fffffffLL || n > 0x7fffffffLL)
            return w2_host_fail(who, "a sign has 2^31 entries or more: tcsc_t offsets are int"), nullptr;
        t = alloc_tcsc(rows, cols, (int)p, (int)n);
        if (!t) return w2_host_fail(who, "out of memory"), nullptr;
        for (int j = 0; j <= cols; ++j) {
            t->col_start_pos[j] = (int)cp[j];
            t->col_start_neg[j] = (int)cn[j];
        }
    }
    return t;
}

// SparseFormat(int* matrix, int K, int N) (SparseGEMM.h:20-39): an int K x N
// matrix, >= 1 stored as +1 and <= -1 as -1 (so 2 and -7 count too, unlike
// tcsc_from_dense's exact compare), rows ascending per column.  Same
// row-major two-pass walk as from_dense_host; the reference walks column by
// column with stride N and produces the same arrays.  Two calls: with
// row_index_* NULL it writes col_start_* (N+1 each) and the counts; then
// with row_index_* sized n_pos / n_neg it fills them.
int tcsc_sparse_format(const int* matrix, int K, int N, int* col_start_pos, int* col_start_neg,
                       int* row_index_pos, int* row_index_neg, int* n_pos, int* n_neg) {
    if (K < 0 || N < 0 || !col_start_pos || !col_start_neg || (!matrix && (long long)K * N > 0)) return TCSC_E_ARG;
    std::vector<long long> cnt_p((size_t)N, 0), cnt_n((size_t)N, 0);
    for (int k = 0; k < K; ++k) {
        const int* r = matrix + (size_t)k * N;
        for (int n = 0; n < N; ++n) {
            cnt_p[n] += (r[n] >= 1);
            cnt_n[n] += (r[n] <= -1);
        }
    }
    long long p = 0, q = 0;
    for (int n = 0; n < N; ++n) {
        col_start_pos[n] = (int)p;
        col_start_neg[n] = (int)q;
        p += cnt_p[n];
        q += cnt_n[n];
        if (p > 0x7fffffffLL || q > 0x7fffffffLL) return TCSC_E_ARG;
    }
    col_start_pos[N] = (int)p;
    col_start_neg[N] = (int)q;
    if (n_pos) *n_pos = (int)p;
    if (n_neg) *n_neg = (int)q;
    if (!row_index_pos || !row_index_neg) return TCSC_OK;
    for (int n = 0; n < N; ++n) {  // cursors
        cnt_p[n] = col_start_pos[n];
        cnt_n[n] = col_start_neg[n];
    }
    for (int k = 0; k < K; ++k) {
        const int* r = matrix + (size_t)k * N;
        for (int n = 0; n < N; ++n) {
            if (r[n] >= 1)
                row_index_pos[cnt_p[n]++] = k;
            else if (r[n] <= -1)
                row_index_neg[cnt_n[n]++] = k;
        }
    }
    return TCSC_OK;
}

void tcsc_set_seed(unsigned long long seed) { g_seed = seed; }

dense_t init_rand_dense(int rows, int cols) {
    const size_t n = (size_t)rows * cols;
    float* m = aligned_floats(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t u = (uint32_t)(splitmix64(&g_seed) >> 40);
        m[i] = (float)u * (1.0f / 8388608.0f) - 1.0f;
    }
    return m;
}

dense_t dense_random(int rows, int cols) { return init_rand_dense(rows, cols); }

dense_t init_rand_sparse(int rows, int cols, int non_zero) {
    const size_t n = (size_t)rows * cols;
    float* m = aligned_floats(n);
    const double d = non_zero > 0 ? 1.0 / non_zero : 0.0, half = 0.5 * d;
    for (size_t i = 0; i < n; ++i) {
        double u = (double)(splitmix64(&g_seed) >> 11) * (1.0 / 9007199254740992.0);
        m[i] = (u < half) ? 1.0f : (u < d ? -1.0f : 0.0f);
    }
    return m;
}

bool compare(const dense_t result, const dense_t target, int rows, int cols) {
    const float tol = 1e-4f;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const size_t ij = (size_t)r * cols + c;
            if (std::fabs(result[ij] - target[ij]) > tol) {
                std::printf("Error at (row, col) = (%d, %d): expected=%f got=%f\n", r, c, target[ij], result[ij]);
                return false;
            }
        }
    return true;
}

// The harness's dense oracle (dense.c:64-77): Y[m,n] = (sum_k X[m,k]*W[k,n])
// + B[n], every element summed from 0 in ascending k with a rounded product
// and a rounded add (no contraction), so the bits equal the reference's IEEE
// build.  Loop order m, k, n (a row of accumulators) instead of m, n, k:
// each element still sees the same sequence of operations, but W is read
// along its rows.  Single-threaded by default, as the reference's (a
// harness that times it as its "GEMM" line, main.cpp:379-391, then compares
// against the same baseline); $TCSC_DENSE_THREADS=n runs row blocks on n
// threads (0 = the usable CPUs, at most 16), same bits.
namespace {
void gemm_rows(const float* X, const float* W, const float* B, float* Y, int m0, int m1, int N, int K) {
#pragma clang fp contract(off)
    constexpr int R = 8;  // rows per pass over W: W is streamed M/R times instead of M times
    std::vector<float> acc((size_t)R * N);
    for (int mb = m0; mb < m1; mb += R) {
        const int r = std::min(R, m1 - mb);
        std::fill(acc.begin(), acc.end(), 0.0f);
        for (int k = 0; k < K; ++k) {
            const float* w = W + (size_t)k * N;
            for (int i = 0; i < r; ++i) {
                const float xv = X[(size_t)(mb + i) * K + k];
                float* a = acc.data() + (size_t)i * N;
                for (int n = 0; n < N; ++n) a[n] = a[n] + xv * w[n];
            }
        }
        for (int i = 0; i < r; ++i) {
            float* y = Y + (size_t)(mb + i) * N;
            const float* a = acc.data() + (size_t)i * N;
            for (int n = 0; n < N; ++n) y[n] = a[n] + B[n];
        }
    }
}
int gemm_threads(int M, int N, int K) {
    const char* env = std::getenv("TCSC_DENSE_THREADS");
    const int want = env ? std::atoi(env) : 1;
    if (want == 1) return 1;
    cpu_set_t set;
    CPU_ZERO(&set);
    int cpus = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : 1;
    // a thread per >= 4 M multiply-adds of work, at most 16 and one per row
    const double work = (double)M * N * K;
    const int cap = want > 1 ? want : std::min(cpus, 16);
    return std::max(1, std::min({cap, M, (int)(work / 4e6) + 1}));
}
}  // namespace

void gemm_basic(const dense_t X, const dense_t W, const dense_t B, dense_t Y, int M, int N, int K) {
    if (M <= 0 || N <= 0) return;
    const int T = gemm_threads(M, N, K);
    if (T == 1) {
        gemm_rows(X, W, B, Y, 0, M, N, K);
        return;
    }
    std::vector<std::thread> th;
    int done = 0;  // rows [0, done) are handed to threads
    try {
        for (int t = 0; t < T; ++t) {
            const int r1 = (int)((long long)M * (t + 1) / T);
            th.emplace_back(gemm_rows, X, W, B, Y, done, r1, N, K);
            done = r1;
        }
    } catch (const std::system_error&) {  // no thread available: the rest on this one
    }
    if (done < M) gemm_rows(X, W, B, Y, done, M, N, K);
    for (auto& x : th) x.join();
}

void gemm_prelu_basic(const dense_t X, const dense_t W, const dense_t B, float a, dense_t Y, int M, int N, int K) {
    gemm_basic(X, W, B, Y, M, N, K);
    for (size_t i = 0; i < (size_t)M * N; ++i) Y[i] = (Y[i] < 0.0f) ? a * Y[i] : Y[i];
}

}  // extern "C"
