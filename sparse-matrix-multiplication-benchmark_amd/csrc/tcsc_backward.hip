// tcsc_backward.hip -- the device half of the backward pass.
//
//  * the index transpose: the TCSC arrays of W[:, c0:c1]^T from those of W, so
//    that dX = dZ . W^T runs on an ordinary plan (k_stream, k_gemm3 and
//    k_small_m unchanged);
//  * k_prelu_bwd: the elementwise half of the layer's backward, dZ = G masked by
//    the forward's own PReLU predicate, and db = the column sums of dZ.
//
// Nothing here adds floats with atomics: the transpose counts with integer
// atomics whose order cannot show in the output (every output column is sorted
// afterwards), and db is summed in one fixed order.
#include <hip/hip_runtime.h>

#include "tcsc_internal.h"

namespace tcsc {

namespace {

int bwd_grid(long long n, int block) {
    long long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 65535LL * 16) g = 65535LL * 16;
    return (int)g;
}

// cnt[k] += 1 for every entry of ri[e0, e0 + n): the length of output column k
__global__ void k_tr_hist(const int* __restrict__ ri, int e0, int n, int* __restrict__ cnt) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        atomicAdd(&cnt[ri[e0 + i]], 1);
}

// One wave per input column j of [col_begin, col_begin + ncols): each of its
// rows k takes the next free place of output column k (cursor[k] starts at the
// column's offset) and stores j - col_begin there.  The places are handed out
// in whatever order the atomics land, so the columns of `out` hold the right
// sets in no particular order; sort_columns puts them in ascending order.
__global__ void __launch_bounds__(256) k_tr_scatter(const int* __restrict__ cs, const int* __restrict__ ri,
                                                     int col_begin, int ncols, int* __restrict__ cursor,
                                                     int* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long j = wave; j < ncols; j += nwaves) {
        const int a = cs[col_begin + j], b = cs[col_begin + j + 1];
        for (int i = a + lane; i < b; i += 64) out[atomicAdd(&cursor[ri[i]], 1)] = (int)j;
    }
}

// ---- k_prelu_bwd -----------------------------------------------------------
// A workgroup owns kBwdCols columns and walks all M rows: kBwdColLanes lanes of
// four columns (one 16-B access) times kBwdRowLanes row-lanes, row-lane r
// taking the rows r, r + kBwdRowLanes, ...  A wave is four row-lanes, so each
// of its accesses covers four 256-B row segments.
constexpr int kBwdCols = 64;
constexpr int kBwdColLanes = kBwdCols / 4;
constexpr int kBwdRowLanes = 32;
constexpr int kBwdThreads = kBwdColLanes * kBwdRowLanes;
constexpr int kBwdUnroll = 4;  // rows in flight per thread

struct Quad {
    float v[4];
};

template <bool VEC>
__device__ __forceinline__ Quad bwd_load(const float* p, int n) {
    Quad q;
    if (VEC && n == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        q.v[0] = t.x, q.v[1] = t.y, q.v[2] = t.z, q.v[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) q.v[i] = i < n ? p[i] : 0.0f;
    }
    return q;
}

template <bool VEC>
__device__ __forceinline__ void bwd_store(float* p, int n, const Quad& q) {
    if (VEC && n == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(q.v[0], q.v[1], q.v[2], q.v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) p[i] = q.v[i];
    }
}

// dZ[m, j] = Y[m, j] < 0 ? a * G[m, j] : G[m, j] (Y null: dZ = G), and
// DB[j] = sum over m of dZ[m, j] in a fixed order: every thread adds its rows
// in ascending m, then the row-lanes are added pairwise in LDS (lane r +=
// lane r + s for s = 16, 8, 4, 2, 1).  DZ may be G or null, DB may be null.
// VEC: every pointer 16-B aligned and every pitch a multiple of 4; the last
// quad of a row with N % 4 != 0 goes element by element either way.
// The product is __fmul_rn so that it is rounded before it is added to the
// column sum (no contraction into an fma): DB sums the stored dZ values.
template <bool VEC>
__global__ void __launch_bounds__(kBwdThreads) k_prelu_bwd(const float* G, size_t ldg, const float* __restrict__ Y,
                                                            size_t ldy, float a, float* DZ, size_t lddz,
                                                            float* __restrict__ DB, int M, int N) {
    __shared__ float red[kBwdRowLanes][kBwdCols];
    const int cl = threadIdx.x % kBwdColLanes, rl = threadIdx.x / kBwdColLanes;
    const long long j0 = (long long)blockIdx.x * kBwdCols + 4 * cl;
    const int n = j0 >= N ? 0 : (N - j0 < 4 ? (int)(N - j0) : 4);  // this thread's columns
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (n > 0) {
        long long m = rl;
        for (; m + (kBwdUnroll - 1) * kBwdRowLanes < M; m += kBwdUnroll * kBwdRowLanes) {
            Quad g[kBwdUnroll], y[kBwdUnroll];
#pragma unroll
            for (int u = 0; u < kBwdUnroll; ++u) {
                const size_t row = (size_t)(m + u * kBwdRowLanes);
                g[u] = bwd_load<VEC>(G + row * ldg + j0, n);
                if (Y) y[u] = bwd_load<VEC>(Y + row * ldy + j0, n);
            }
#pragma unroll
            for (int u = 0; u < kBwdUnroll; ++u) {
                const size_t row = (size_t)(m + u * kBwdRowLanes);
                if (Y) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (y[u].v[i] < 0.0f) g[u].v[i] = __fmul_rn(a, g[u].v[i]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += g[u].v[i];
                if (DZ) bwd_store<VEC>(DZ + row * lddz + j0, n, g[u]);
            }
        }
        for (; m < M; m += kBwdRowLanes) {
            Quad g = bwd_load<VEC>(G + (size_t)m * ldg + j0, n);
            if (Y) {
                const Quad y = bwd_load<VEC>(Y + (size_t)m * ldy + j0, n);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (y.v[i] < 0.0f) g.v[i] = __fmul_rn(a, g.v[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] += g.v[i];
            if (DZ) bwd_store<VEC>(DZ + (size_t)m * lddz + j0, n, g);
        }
    }
    if (!DB) return;  // uniform: no barrier is skipped by part of a workgroup
#pragma unroll
    for (int i = 0; i < 4; ++i) red[rl][4 * cl + i] = acc[i];
    __syncthreads();
    for (int s = kBwdRowLanes / 2; s >= 1; s >>= 1) {
        if (rl < s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) red[rl][4 * cl + i] += red[rl + s][4 * cl + i];
        }
        __syncthreads();
    }
    if (rl == 0) {
        for (int i = 0; i < n; ++i) DB[j0 + i] = red[0][4 * cl + i];
    }
}

}  // namespace

hipError_t transpose_sign(const int* cs, const int* ri, int col_begin, int ncols, int rows, int e0, int n, int* cnt,
                          int* cursor, int* unsorted, void* tmp, size_t tmp_bytes, int* t_cs, int* t_ri,
                          hipStream_t st) {
    hipError_t e;
    if ((e = hipMemsetAsync(cnt, 0, (size_t)(rows + 1) * sizeof(int), st)) != hipSuccess) return e;
    if (n > 0) {
        hipLaunchKernelGGL(k_tr_hist, dim3(bwd_grid(n, 256)), dim3(256), 0, st, ri, e0, n, cnt);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = exclusive_scan_i32(cnt, t_cs, rows + 1, tmp, tmp_bytes, st)) != hipSuccess) return e;
    if (n <= 0 || rows <= 0) return hipSuccess;
    if ((e = hipMemcpyAsync(cursor, t_cs, (size_t)rows * sizeof(int), hipMemcpyDeviceToDevice, st)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_tr_scatter, dim3(bwd_grid((long long)ncols * 64, 256)), dim3(256), 0, st, cs, ri, col_begin,
                       ncols, cursor, unsorted);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return sort_columns(unsorted, t_ri, n, rows, t_cs, tmp, tmp_bytes, st);
}

hipError_t launch_prelu_bwd(const float* G, int ldg, const float* Y, int ldy, float a, float* DZ, int lddz, float* DB,
                            int M, int N, hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = al(G) && ldg % 4 == 0 && (!Y || (al(Y) && ldy % 4 == 0)) && (!DZ || (al(DZ) && lddz % 4 == 0));
    const dim3 grid((unsigned)(((long long)N + kBwdCols - 1) / kBwdCols));
    if (vec)
        hipLaunchKernelGGL(k_prelu_bwd<true>, grid, dim3(kBwdThreads), 0, st, G, (size_t)ldg, Y, (size_t)ldy, a, DZ,
                           (size_t)lddz, DB, M, N);
    else
        hipLaunchKernelGGL(k_prelu_bwd<false>, grid, dim3(kBwdThreads), 0, st, G, (size_t)ldg, Y, (size_t)ldy, a, DZ,
                           (size_t)lddz, DB, M, N);
    return hipGetLastError();
}

}  // namespace tcsc
