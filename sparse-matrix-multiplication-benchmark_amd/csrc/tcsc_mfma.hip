// tcsc_mfma.hip -- the MFMA path for near-dense W.
//
// At 50 % density (BASELINE cfg 5) the gather walks half of W: 33.5 M
// nonzeros x 2048 rows at ~27 T adds/s = 2.5 ms, while the matrix cores
// multiply the dense W far faster in bf16.  The path keeps fp32 results
// without an fp32 MFMA (the fp32 matrix rate is the vector rate): every x is
// split exactly into three bf16 parts, x = h + m + l (truncations of x and of
// its remainders: 8 + 8 + 8 significand bits), W is exact in bf16 (0, +-1,
// or small integers for duplicate rows), so each product is exact and the
// GEMM
//     Y = [h | m | l] . [W ; W ; W]           (M x 3K) . (3K x N)
// accumulates in fp32 on the matrix cores -- k_gemm3, written here for
// gfx950: 256 x 256 tiles of 8 waves (v_mfma_f32_16x16x32_bf16), X3 (M x ldk,
// [h | m | l] per 64-k block) and W^T (N x ldw, stored once) staged into LDS
// rings by LDS-DMA with a conflict-free swizzle, each W block multiplied with
// the three parts of its X3 block in turn, bias (+ PReLU) fused into the
// store.  Only the summation order differs from the gather's: the result is
// within the fast-order bound, and bit-exact on integer-valued inputs.
//
// Rows the split cannot carry are recomputed by the gather order: a
// non-finite x would make inf*0 = NaN in columns whose W is 0 there (the
// reference never touches those products), and bf16 MFMA inputs below
// 2^-126 may be flushed.  k_split3 flags every row holding a non-finite x
// or a nonzero |x| < 2^-100 (it writes every row's flag on every call, so a
// captured graph replays correctly); k_fixup rewrites those rows from the
// plan's merged per-column CSC copy, +1 and -1 rows in ascending k (+1 first
// on a tie), then the bias, then the PReLU -- the exact arithmetic of
// k_stream's fast order (= the reference's dense.c gemm_basic order).  It
// rebuilds x from X3, so a tiny x, whose low bits no bf16 can hold, is stored
// there as its bits (split3).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "tcsc_i8_out.h"
#include "tcsc_internal.h"
#include "tcsc_norm.h"
#include "tcsc_quant.h"
#include "tcsc_w2.h"
#include "tcsc_xsrc.h"

namespace tcsc {
namespace {

inline int grid_of(long long n, int block) {
    long long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 65535LL * 16) g = 65535LL * 16;
    return (int)g;
}

__device__ inline uint32_t f2u(float x) { return __float_as_uint(x); }
__device__ inline float u2f(uint32_t u) { return __uint_as_float(u); }

// x -> (h, m, l) bf16 bit patterns with h + m + l == x exactly (finite x of
// magnitude >= 2^-100); a non-finite x goes whole into h (a quiet NaN keeps
// its sign), m = l = 0.  A nonzero |x| < 2^-100 is stored as its bits, h the
// high and m the low 16 (l = 0): its remainders fall below bf16's range (x -
// h is an fp32 denormal from 2^-118 down, and nothing under 2^-133 is a bf16
// at all), so three truncations would lose them.  Its row is flagged, the
// GEMM's sums for it are discarded, and exact_out() reassembles the bits (it
// tells the two forms apart by h's exponent: below 2^-100 or not).
// Returns whether the row needs the exact fixup.
constexpr uint32_t kTinyExp = 27;  // biased exponent of 2^-100
__device__ inline bool split3(float x, uint16_t& h, uint16_t& m, uint16_t& l) {
    const uint32_t u = f2u(x);
    if ((u & 0x7f800000u) == 0x7f800000u) {  // inf or NaN
        const bool nan = (u & 0x007fffffu) != 0;
        h = (uint16_t)(nan ? ((u >> 16) | 0x0040u) : (u >> 16));
        m = l = 0;
        return true;
    }
    if (x != 0.0f && ((u >> 23) & 0xffu) < kTinyExp) {  // 0 < |x| < 2^-100
        h = (uint16_t)(u >> 16);
        m = (uint16_t)u;
        l = 0;
        return true;
    }
    const uint32_t hu = u & 0xffff0000u;
    const float r = x - u2f(hu);              // exact: the low 16 bits of x
    const uint32_t mu = f2u(r) & 0xffff0000u;
    const float s = r - u2f(mu);              // exact: at most 8 significant bits left
    h = (uint16_t)(hu >> 16);
    m = (uint16_t)(mu >> 16);
    l = (uint16_t)(f2u(s) >> 16);
    return false;
}

// X (M x K, pitch K) -> X3 (M x ldk bf16): [h | m | l | 0 ...] per row, one
// workgroup per row; flags[row] = 1 when the fixup must recompute the row,
// else 0 (written every call).  A thread loads kSplitU 16-B pieces before it
// splits and stores any of them: at small M (one workgroup per row, few rows)
// the row's loads then overlap instead of running as kq / 256 dependent round
// trips (M = 64, K = 8192: 11.3 us before).
constexpr int kSplitU = 8;
__global__ void __launch_bounds__(256) k_split3(const float* __restrict__ X, int M, int K, uint16_t* __restrict__ X3,
                                               int ldk, int* __restrict__ flags) {
    const int row = blockIdx.x;
    const float* src = X + (size_t)row * K;
    uint16_t* dst = X3 + (size_t)row * ldk;
    const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    bool fix = false;
    const int kq = (K + 3) / 4;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
    if (vec) {
        for (int q0 = threadIdx.x; q0 < kq; q0 += kSplitU * blockDim.x) {
            f4 w[kSplitU];
#pragma unroll
            for (int u = 0; u < kSplitU; ++u) {
                const int q = q0 + u * blockDim.x;
                if (q < kq) w[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src + 4 * q));
            }
#pragma unroll
            for (int u = 0; u < kSplitU; ++u) {
                const int q = q0 + u * blockDim.x;
                if (q >= kq) break;
                const int k0 = 4 * q;  // k0 .. k0+3 lie in one block
                uint16_t h[4], m[4], l[4];
                for (int j = 0; j < 4; ++j) fix |= split3(w[u][j], h[j], m[j], l[j]);
                *reinterpret_cast<u16x4*>(dst + x3_index(k0, 0)) = u16x4{h[0], h[1], h[2], h[3]};
                *reinterpret_cast<u16x4*>(dst + x3_index(k0, 1)) = u16x4{m[0], m[1], m[2], m[3]};
                *reinterpret_cast<u16x4*>(dst + x3_index(k0, 2)) = u16x4{l[0], l[1], l[2], l[3]};
            }
        }
    } else {
        for (int q = threadIdx.x; q < kq; q += blockDim.x) {
            const int k0 = 4 * q;
            float v[4];
            for (int j = 0; j < 4; ++j) v[j] = k0 + j < K ? src[k0 + j] : 0.0f;
            uint16_t h[4], m[4], l[4];
            for (int j = 0; j < 4; ++j) fix |= split3(v[j], h[j], m[j], l[j]);
            for (int j = 0; j < 4 && k0 + j < K; ++j) {
                dst[x3_index(k0 + j, 0)] = h[j];
                dst[x3_index(k0 + j, 1)] = m[j];
                dst[x3_index(k0 + j, 2)] = l[j];
            }
        }
    }
    // zeros past K: the last block's tail in each part, then the row pad
    const int tail0 = (mfma_nblk(K) - 1) * 3 * kMfmaBlk;
    for (int i = tail0 + threadIdx.x; i < ldk; i += blockDim.x)
        if (i >= 3 * kMfmaBlk * mfma_nblk(K) || (mfma_nblk(K) - 1) * kMfmaBlk + i % kMfmaBlk >= K) dst[i] = 0;
    fix = __syncthreads_or(fix);
    if (threadIdx.x == 0) flags[row] = fix ? 1 : 0;
}

// k_split3's flag rule on a bf16 x (its fp32 value is bits << 16): non-finite,
// or nonzero below 2^-100.  The same rows are flagged as by split3 on the
// widened x.
__device__ inline bool flag1(uint32_t b) {
    const uint32_t e = (b >> 7) & 0xffu;
    return e == 0xffu || ((b & 0x7fffu) != 0 && e < kTinyExp);
}

// bf16 X (M x K, pitch K) -> X1 (M x ldw bf16): the row as it is, zeros past
// K (the W image's pitch: whole 64-k blocks), one workgroup per row; flags[row]
// as k_split3 writes it (every row, every call).  A flagged x stays its own
// bits.  VEC (K % 8 == 0, X 16-B aligned): kSplitU 16-B loads (8 bf16 each) in
// flight per thread, 16-B stores; otherwise scalar.
__global__ void __launch_bounds__(256) k_pack1(const uint16_t* __restrict__ X, int M, int K, uint16_t* __restrict__ X1,
                                              int ldw, int* __restrict__ flags) {
    const int row = blockIdx.x;
    const uint16_t* src = X + (size_t)row * K;
    uint16_t* dst = X1 + (size_t)row * ldw;
    const bool vec = (K & 7) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    bool fix = false;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (vec) {
        const int ko = K / 8;
        for (int q0 = threadIdx.x; q0 < ko; q0 += kSplitU * blockDim.x) {
            u32x4 w[kSplitU];
#pragma unroll
            for (int u = 0; u < kSplitU; ++u) {
                const int q = q0 + u * blockDim.x;
                if (q < ko) w[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + 8 * q));
            }
#pragma unroll
            for (int u = 0; u < kSplitU; ++u) {
                const int q = q0 + u * blockDim.x;
                if (q >= ko) break;
                for (int j = 0; j < 4; ++j) fix |= flag1(w[u][j] & 0xffffu) || flag1(w[u][j] >> 16);
                *reinterpret_cast<u32x4*>(dst + 8 * q) = w[u];
            }
        }
    } else {
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            const uint16_t b = src[k];
            fix |= flag1(b);
            dst[k] = b;
        }
    }
    for (int i = K + threadIdx.x; i < ldw; i += blockDim.x) dst[i] = 0;
    fix = __syncthreads_or(fix);
    if (threadIdx.x == 0) flags[row] = fix ? 1 : 0;
}

// The +1/-1 entries of column j (rebased CSC) added into a dense fp32 image
// of W^T (ncols x K, k contiguous; atomics: a row may repeat in a column).
__global__ void k_w_scatter(const int* __restrict__ cs, const int* __restrict__ ri, int col_begin, int ncols,
                            int K, float sign, float* __restrict__ WfT) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= ncols) return;
    const int base = cs[col_begin];
    const int e0 = cs[col_begin + j] - base, e1 = cs[col_begin + j + 1] - base;
    const int* r = ri + base;
    for (int e = e0 + lane; e < e1; e += 64) atomicAdd(&WfT[(size_t)j * K + r[e]], sign);
}

// WfT (ncols x K fp32) -> WT (ncols x ldw bf16, the pad zeroed before), k
// contiguous like X3.  Values must be integers of magnitude <= 256 to be
// exact in bf16; *bad = 1 otherwise.
__global__ void k_wt_from(const float* __restrict__ WfT, int ncols, int K, uint16_t* __restrict__ WT, int ldw,
                          int* __restrict__ bad) {
    const long long n = (long long)ncols * K;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const float w = WfT[i];
        if (fabsf(w) > 256.0f) *bad = 1;
        const long long j = i / K, k = i - j * K;
        WT[j * ldw + k] = (uint16_t)(f2u(w) >> 16);
    }
}

// dst[e] = src[base + e], base = cs[col_begin] (the column range's first entry)
__global__ void k_copy_from(const int* __restrict__ src, const int* __restrict__ cs, int col_begin, long long n,
                            int* __restrict__ dst) {
    const int base = cs[col_begin];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        dst[i] = src[base + i];
}

// gq[g] = quads of group g: its longest column's entries over 4, rounded up
// to a multiple of 16 quads (the small-M kernel's unroll); gq[groups] = 0.
__global__ void k_group_quads(const int* __restrict__ cp, const int* __restrict__ cn, int ncols,
                              int* __restrict__ gq) {
    const int ng = csc_groups(ncols);
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g <= ng; g += gridDim.x * blockDim.x) {
        int mx = 0;
        if (g < ng)
            for (int j = g * kCscGroup; j < min(ncols, (g + 1) * kCscGroup); ++j)
                mx = max(mx, cp[j + 1] - cp[j] + cn[j + 1] - cn[j]);
        gq[g] = g < ng ? ((mx + 3) / 4 + 15) & ~15 : 0;
    }
}

// Merge each column's +1 and -1 rows (rebased lists rp / rn, offsets cp /
// cn) into one list in ascending row order -- entries 4*row for +1 rows and
// csc_neg_base(rows) + 4*row for -1 rows, a +1 entry first on a tie (k_scatter's
// rule) -- in the quad layout, padded to its group's length with 4*rows
// entries: the order in which k_stream's fast order adds a column's nonzeros.
__global__ void k_merge_csc(const int* __restrict__ cp, const int* __restrict__ cn, const int* __restrict__ rp,
                            const int* __restrict__ rn, const int* __restrict__ cq, int ncols, int rows,
                            int* __restrict__ rm) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ncols; j += gridDim.x * blockDim.x) {
        const int g = j / kCscGroup;
        const int n = 4 * (cq[g + 1] - cq[g]);
        int p = cp[j], q = cn[j], i = 0;
        const int p1 = cp[j + 1], q1 = cn[j + 1];
        while (p < p1 || q < q1) {
            int e;
            if (q >= q1 || (p < p1 && rp[p] <= rn[q]))
                e = 4 * rp[p++];
            else
                e = csc_neg_base(rows) + 4 * rn[q++];
            rm[csc_entry(cq, j, i++)] = e;
        }
        for (; i < n; ++i) rm[csc_entry(cq, j, i)] = 4 * rows;
    }
}

// Output (row, j) recomputed exactly as k_stream's fast order (see the file
// comment): x rebuilt from its three parts (or its stored bits), the column's merged rows in
// ascending k, the bias first or last, then the PReLU.  PARTS = 1: X3 is the
// one-part image X1 (pitch ldk = mfma_ldw(K)) and x is its bf16 widened, a
// flagged tiny x included (it is its own bits).
template <bool BIAS_FIRST, bool PRELU, int PARTS = 3>
__device__ inline float exact_out(const uint16_t* __restrict__ X3, int K, int ldk, const int* __restrict__ cq,
                                  const int* __restrict__ rm, const float* __restrict__ Bias, int row, int j,
                                  float a) {
    const uint16_t* x3 = X3 + (size_t)row * ldk;
    auto xk = [&](int k) {
        if constexpr (PARTS == 1) return u2f((uint32_t)x3[k] << 16);
        // all three loads, then a select: no branch in the column walk
        const uint32_t hb = x3[x3_index(k, 0)], mb = x3[x3_index(k, 1)], lb = x3[x3_index(k, 2)];
        const float sum = (u2f(hb << 16) + u2f(mb << 16)) + u2f(lb << 16);
        return (hb & 0x7f80u) < (kTinyExp << 7) ? u2f(hb << 16 | mb) : sum;  // |x| < 2^-100 (or 0): its bits
    };
    float acc = BIAS_FIRST ? Bias[j] : 0.0f;
    const int g = j / kCscGroup, n = 4 * (cq[g + 1] - cq[g]);
    for (int i = 0; i < n; ++i) {
        const int r = rm[csc_entry(cq, j, i)];
        if (r == 4 * K) break;  // the column's padding
        const bool neg = r >= csc_neg_base(K);
        const int k = (neg ? r - csc_neg_base(K) : r) >> 2;
        acc = fmaf(xk(k), neg ? -1.0f : 1.0f, acc);
    }
    if (!BIAS_FIRST) acc += Bias[j];
    if (PRELU) acc = (acc < 0.0f) ? a * acc : acc;
    return acc;
}

// Flagged rows, after the GEMM (which wrote act(sum + bias) for every row):
// one thread per column.  A block first ORs the row flags; most calls have
// none and the kernel ends there.
template <bool BIAS_FIRST, bool PRELU, int PARTS = 3>
__global__ void __launch_bounds__(256) k_fixup(const uint16_t* __restrict__ X3, int M, int K, int ldk,
                                               const int* __restrict__ cq, const int* __restrict__ rm,
                                               int ncols,
                                               const float* __restrict__ Bias, float* __restrict__ Y, int ldy, float a,
                                               const int* __restrict__ flags) {
    int any = 0;
    for (int r = threadIdx.x; r < M; r += blockDim.x) any |= flags[r];
    if (!__syncthreads_or(any)) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ncols) return;
    for (int row = 0; row < M; ++row)
        if (flags[row])
            Y[(size_t)row * ldy + j] = exact_out<BIAS_FIRST, PRELU, PARTS>(X3, K, ldk, cq, rm, Bias, row, j, a);
}

// ---------------------------------------------------------------------------
// k_gemm3: Y[m, n] = act(sum_k A[m, k] * Bt[n, k] + bias[n]), bf16 in, fp32
// accumulate, A = X3 (M x ldk: [h | m | l] per 64-k block), Bt = WT (N x ldw:
// W's block once).
//
// * Tile TM x TN = (WM*FI*16) x (WN*FJ*16) per workgroup of WM*WN waves; a
//   wave owns FI x FJ blocks of 16 x 16 (v_mfma_f32_16x16x32_bf16, 4 fp32
//   accumulators per lane per block).  128 x 512 with 8 waves (1 x 8, 128 x
//   64 per wave) for the large shapes; 128 x 128 with 4 waves for grids that
//   would leave CUs idle.
// * The k loop runs over sub-steps (block, part): one part of X3's 64-k
//   block against W's block.  A is staged per sub-step in a 2-slot ring, W
//   once per block in a 2-slot ring of its own, by LDS-DMA
//   (global_load_lds_dwordx4: 1 KiB per wave-instruction, no VGPRs).  The
//   GEMM is bound by that staging (L2 -> LDS, ~43 GB/s per CU): staging W once
//   per block instead of with every part moves 1/3 fewer bytes per MFMA.
// * LDS image of a slot: 1-KiB pieces of 8 rows x 64
//   k (128 B per row).  Inside a piece the 16-B granule g (8 k) of row r sits
//   at slot 8r + (g ^ r): the DMA writes the piece lane-linear (lane = slot)
//   from per-lane source addresses, and the MFMA fragment reads (lane l:
//   row l & 15 of a 16-row block, granule 4*kh + l/16) then hit 16 distinct
//   16-B slots in every ds_read_b128 lane group: conflict-free (4 LDS
//   cycles per read instead of 16-32 for a linear image).
// * Rows past M / N load the last valid row (in bounds) and are not stored.
// * Tile order: XCD-aware and bijective; an XCD's ~32 concurrent workgroups
//   take 4 row tiles x 8 column tiles, sharing A and W tiles in its L2.
// ---------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Split K (k_gemm3 PARTIAL): the slabs added in slice order, then the bias,
// then the PReLU -- k_reduce4's arithmetic, element for element -- with
// k_fixup folded in: a flagged row takes exact_out() instead, so a split call
// needs no fixup launch.  VEC: 4 columns per thread (N % 4 == 0, ldy % 4 ==
// 0, 16-B aligned slabs, bias and Y), all slices' loads in flight.
template <bool PRELU, bool VEC, int PARTS = 3>
__global__ void __launch_bounds__(256) k_reduce_fix(const float* __restrict__ ws, int slices, int M, int N,
                                                    const float* __restrict__ Bias, float* __restrict__ Y, int ldy,
                                                    float a, const int* __restrict__ flags,
                                                    const uint16_t* __restrict__ X3, int K, int ldk,
                                                    const int* __restrict__ cq, const int* __restrict__ rm) {
    constexpr int W = VEC ? 4 : 1;
    const int nq = N / W;
    const long long total = (long long)M * nq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(i / nq), col = W * (int)(i % nq);
        float v[W];
        if (flags[row]) {
#pragma unroll
            for (int u = 0; u < W; ++u) v[u] = exact_out<false, PRELU, PARTS>(X3, K, ldk, cq, rm, Bias, row, col + u, a);
        } else {
            const size_t slab = (size_t)M * N, e = (size_t)row * N + col;
            float p[16][W];
#pragma unroll
            for (int s = 0; s < 16; ++s)
                if (s < slices) {
                    if constexpr (VEC) {
                        const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ws + s * slab + e));
#pragma unroll
                        for (int u = 0; u < 4; ++u) p[s][u] = q[u];
                    } else {
                        p[s][0] = ws[s * slab + e];
                    }
                }
#pragma unroll
            for (int u = 0; u < W; ++u) {
                float t = 0.f;
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    if (s < slices) t += p[s][u];
                t += Bias[col + u];
                if (PRELU) t = (t < 0.0f) ? a * t : t;
                v[u] = t;
            }
        }
        float* dst = Y + (size_t)row * ldy + col;
        if constexpr (VEC) {
            const f32x4 o = {v[0], v[1], v[2], v[3]};
            __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(dst));
        } else {
            dst[0] = v[0];
        }
    }
}


// XCD-aware bijective renumbering of blockIdx.x (an XCD's workgroups get
// consecutive numbers), then bands of gm row tiles walked column by column:
// an XCD's ~32 concurrent workgroups take gm row tiles x 32 / gm column
// tiles, sharing those A and W tiles in its L2.
template <int TM, int TN>
__device__ __forceinline__ void gemm3_tile(int tiles_m, int tiles_n, int gm, int& m0, int& n0) {
    const int T = tiles_m * tiles_n, L = blockIdx.x;
    const int q = T >> 3, r = T & 7, x = L & 7;
    const int Lg = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (L >> 3);
    const int band = Lg / (gm * tiles_n), rb = Lg - band * gm * tiles_n;
    const int g = min(gm, tiles_m - band * gm);  // the last band may be shorter
    m0 = (band * gm + rb % g) * TM;
    n0 = (rb / g) * TN;
}

// The k_gemm3 epilogue (both staging forms): Y = act(acc + bias) for the
// workgroup's tile, the raw sums parked in the LDS (LDSB bytes, free once the
// k loop has drained) and stored as whole rows.
// PARTS only names the caller: each k_gemm3 form gets its own instance, so
// adding the one-part kernels leaves the three-part ones' code as it was (a
// shared instance changed how the epilogue's addresses were folded).
template <int WM, int WN, int FI, int FJ, bool PRELU, bool BIAS, int LDSB, int PARTS>
__device__ __forceinline__ void gemm3_store(const f32x4 (&acc)[FI][FJ], char* lds, int lane, int wr, int wc, int m0,
                                            int n0, int M, int N, const float* __restrict__ bias,
                                            float* __restrict__ Y, int ldy, float a) {
    constexpr int TM = WM * FI * 16, TN = WN * FJ * 16, NW = WM * WN;
    // Epilogue: lane l holds rows 4*(l/16) + reg, column l % 16 of each 16 x 16
    // block.  Stored as is, one instruction would write 4 rows x 16 columns of
    // 4-B pieces (store-issue-bound); instead each pass of 64 tile rows is
    // parked in the (now free) LDS, row stride TN + 4 floats (the 4 row groups
    // of a block fall 16 banks apart), and read back as whole rows: 16-B
    // stores, TN / 4 lanes per row.  Same values, same bits.
    constexpr int PR = 64, SROW = TN + 4, LPR = TN / 4;  // rows per pass, staged row, lanes per row
    static_assert(PR * SROW * 4 <= LDSB && TM % PR == 0 && (64 % LPR == 0 || LPR % 64 == 0), "epilogue staging");
    // (the raw sums are parked; bias and PReLU are applied to the rows read
    // back, where a lane's 4 columns stay the same: NW * 64 is a multiple of LPR)
    static_assert((NW * 64) % LPR == 0, "a lane keeps its columns across the read-back");
    float* stg = reinterpret_cast<float*>(lds);
    const bool vec = (ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0;
    const int c4 = 4 * (threadIdx.x % LPR), col = n0 + c4;
    f32x4 bq = f32x4{0.f, 0.f, 0.f, 0.f};
    if (BIAS)
#pragma unroll
        for (int u = 0; u < 4; ++u) bq[u] = col + u < N ? bias[col + u] : 0.0f;
#pragma unroll
    for (int p = 0; p < TM / PR; ++p) {
#pragma unroll
        for (int i = 0; i < FI; ++i) {
            if (((wr * FI + i) * 16) / PR != p) continue;  // uniform
            const int rb = (wr * FI + i) * 16 - p * PR + 4 * (lane >> 4);
#pragma unroll
            for (int j = 0; j < FJ; ++j) {
                const int c = (wc * FJ + j) * 16 + (lane & 15);
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) stg[(rb + rg) * SROW + c] = acc[i][j][rg];
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < PR * LPR; e += NW * 64) {
            const int r = e / LPR;
            const int row = m0 + p * PR + r;
            if (row >= M) continue;
            f32x4 v = *reinterpret_cast<const f32x4*>(stg + r * SROW + c4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (BIAS) v[u] = v[u] + bq[u];
                if (PRELU) v[u] = (v[u] < 0.0f) ? a * v[u] : v[u];
            }
            float* dst = Y + (size_t)row * ldy + col;
            if (vec && col + 3 < N) {
                __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst));
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (col + u < N) __builtin_nontemporal_store(v[u], dst + u);
            }
        }
        __syncthreads();  // the staging is reused by the next pass
    }
}

// PARTIAL (split-K, blockIdx.y = the slice): the workgroup walks 64-k blocks
// [y * bps, min(nblk, (y + 1) * bps)) and stores its raw fp32 sums into slab
// y of Y (M x ldy floats per slab); k_reduce4 adds the slabs in slice order,
// then the bias and the PReLU.
//
// PARTS = 1 (bf16 X, tcsc_gpu_sgemm_bf16): A = X1 (M x ldk, ldk = mfma_ldw(K):
// the row itself in 64-k blocks), every sub-step a whole block: A and W are
// both staged per sub-step into their 2-slot rings and W's fragments are read
// every sub-step.  Same tiles, swizzle, half-step pipeline and epilogue.
template <int WM, int WN, int FI, int FJ, bool PRELU, bool PARTIAL, int PARTS = 3>
__global__ void __launch_bounds__(WM * WN * 64) k_gemm3(const uint16_t* __restrict__ A, const uint16_t* __restrict__ Bt,
                                                      int ldk, int ldw, int M, int N, int nblk,
                                                      const float* __restrict__ bias, float* __restrict__ Y, int ldy,
                                                      float a, int tiles_m, int tiles_n, int gm, int bps) {
    static_assert(!(PARTIAL && PRELU), "a partial slab carries raw sums");
    static_assert(PARTS == 3 || PARTS == 1, "three bf16 parts of an fp32 x, or a bf16 x");
    constexpr int TM = WM * FI * 16, TN = WN * FJ * 16, NW = WM * WN;
    constexpr int PA = TM / 8, PB = TN / 8;  // 1-KiB pieces of a slot
    constexpr int ASLOT = PA * 1024, BSLOT = PB * 1024, BOFF = 2 * ASLOT;
    constexpr int PAW = PA / NW, PBW = PB / NW;  // pieces each wave moves per A / B slot
    static_assert(PA % NW == 0 && PB % NW == 0, "whole pieces per wave");
    __shared__ __attribute__((aligned(1024))) char lds[2 * ASLOT + 2 * BSLOT];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave / WN, wc = wave % WN;

    int m0, n0;
    gemm3_tile<TM, TN>(tiles_m, tiles_n, gm, m0, n0);

    // this wave's DMA pieces: a uniform base (the operand's tile) plus per-lane
    // byte offsets (rows clamped into the matrix; 32-bit: the saddr form)
    const int row_in = lane >> 3, gsel = (lane & 7) ^ row_in;
    uint32_t offa[PAW];
#pragma unroll
    for (int i = 0; i < PAW; ++i)
        offa[i] = 2u * (uint32_t)(min(8 * (wave * PAW + i) + row_in, M - 1 - m0) * ldk + 8 * gsel);
    const char* abase = reinterpret_cast<const char*>(A + (size_t)m0 * ldk);
    const char* bbase = reinterpret_cast<const char*>(Bt + (size_t)n0 * ldw);
    auto dma_a = [&](int blk, int part, int slot) {  // X3's part `part` of 64-k block `blk`
        const char* g = abase + 2 * (size_t)(kMfmaBlk * (PARTS * blk + part));
#pragma unroll
        for (int i = 0; i < PAW; ++i)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(g + offa[i]),
                                             (__attribute__((address_space(3))) void*)(lds + slot * ASLOT +
                                                                                       (wave * PAW + i) * 1024),
                                             16, 0, 0);
    };
    auto dma_b = [&](int blk, int slot) {  // W's 64-k block `blk` (offsets recomputed: once per block)
        const char* g = bbase + 2 * (size_t)(kMfmaBlk * blk);
#pragma unroll
        for (int i = 0; i < PBW; ++i)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(
                                                 g + 2u * (uint32_t)(min(8 * (wave * PBW + i) + row_in, N - 1 - n0) * ldw +
                                                                     8 * gsel)),
                                             (__attribute__((address_space(3))) void*)(lds + BOFF + slot * BSLOT +
                                                                                       (wave * PBW + i) * 1024),
                                             16, 0, 0);
    };

    // fragment read offsets inside a 16-row block (the swizzle above)
    int foff[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
        foff[kh] = ((lane & 15) >> 3) * 1024 + 16 * (8 * (lane & 7) + ((4 * kh + (lane >> 4)) ^ (lane & 7)));

    f32x4 acc[FI][FJ];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Half-step pipeline: the fragments of the two k halves live in two
    // register sets, and the one barrier per sub-step sits between them.
    // Sub-step s (block s / 3, part s % 3; A slot s & 1, B slot block & 1):
    //   read kh 1 of s (set 1)  |  MFMAs on set 0 (kh 0 of s)
    //   wait: set 1 read, DMA of s+1 landed; barrier (every wave is done with
    //   s's A slot -- and, at a block's first part, with the previous block's
    //   B slot -- and s+1 is in LDS)
    //   DMA A of s+2 into s's slot (+ the next block's B at a first part),
    //   read kh 0 of s+1 (set 0)  |  MFMAs on set 1
    // so each wave leaves the barrier with 32 MFMAs whose operands are already
    // in registers, and the DMA issue and the next reads run under them.
    // W's fragments are the same for a block's three parts: set kh of bfr is
    // read at the block's first part and kept through its last (A's are read
    // every sub-step).
    bf16x8 af[2][FI], bfr[2][FJ];
    auto frag_a = [&](int set, int aslot, int kh) {
        const char* sa = lds + aslot * ASLOT;
#pragma unroll
        for (int i = 0; i < FI; ++i)
            af[set][i] = *reinterpret_cast<const bf16x8*>(sa + ((wr * FI + i) * 2) * 1024 + foff[kh]);
    };
    auto frag_b = [&](int set, int bslot, int kh) {
        const char* sb = lds + BOFF + bslot * BSLOT;
#pragma unroll
        for (int j = 0; j < FJ; ++j)
            bfr[set][j] = *reinterpret_cast<const bf16x8*>(sb + ((wc * FJ + j) * 2) * 1024 + foff[kh]);
    };
    auto mma = [&](int set) {
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
            for (int j = 0; j < FJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[set][i], bfr[set][j], acc[i][j], 0, 0, 0);
    };

    // The order is pinned (the compiler otherwise hoists the barrier over the
    // MFMAs and issues every read and DMA piece in one burst): each half step
    // is one scheduling region, one read per MFMA pair.  The tail's DMA is
    // clamped to the last block (a harmless reload into a slot no one reads
    // again) and its extra fragment read is discarded.
    constexpr int NM = FI * FJ;
    static_assert(2 * (FI + FJ) <= NM, "one read per MFMA pair");
    auto pin = [&](auto nr_c) {  // nr reads, one per MFMA pair, then the rest of the MFMAs
        constexpr int NR = decltype(nr_c)::value;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA (first: its operands are the older reads)
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
        }
        if constexpr (NM > 2 * NR) __builtin_amdgcn_sched_group_barrier(0x008, NM - 2 * NR, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    using with_b = std::integral_constant<int, FI + FJ>;
    using a_only = std::integral_constant<int, FI>;
    // this workgroup's 64-k blocks (the host makes every slice non-empty);
    // ring slots count from the first of them
    const int b0 = PARTIAL ? (int)blockIdx.y * bps : 0;
    const int b1 = PARTIAL ? min(nblk, b0 + bps) : nblk;
    const int last = b1 - 1;
    if constexpr (PARTS == 3) {
        dma_a(b0, 0, 0);
        dma_b(b0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        dma_a(b0, 1, 1);
        frag_b(0, 0, 0);
        frag_a(0, 0, 0);
        for (int blk = b0; blk < b1; ++blk) {
            const int bs = (blk - b0) & 1;
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                const int as = (blk - b0 + part) & 1;  // (3 * (blk - b0) + part) & 1
                if (part == 0) frag_b(1, bs, 1);
                frag_a(1, as, 1);
                mma(0);
                if (part == 0) pin(with_b{}); else pin(a_only{});
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
                // A of sub-step s + 2: (blk, 2) after part 0, else (blk + 1, part - 1)
                if (part == 0) {
                    dma_a(blk, 2, as);
                    dma_b(min(blk + 1, last), bs ^ 1);
                } else {
                    const bool tail = blk == last;  // uniform: a scalar select, no branch
                    dma_a(tail ? last : blk + 1, tail ? 2 : part - 1, as);
                }
                if (part == 2) frag_b(0, bs ^ 1, 0);  // the next block's
                frag_a(0, as ^ 1, 0);
                mma(1);
                if (part == 2) pin(with_b{}); else pin(a_only{});
            }
        }
    } else {
        // One part: sub-step s = blk - b0, A and W slots s & 1.  The same
        // half steps; both carry W's reads (with_b), and the DMA after the
        // barrier brings A and W of block s + 2 into the slots s just left.
        dma_a(b0, 0, 0);
        dma_b(b0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        dma_a(min(b0 + 1, last), 0, 1);
        dma_b(min(b0 + 1, last), 1);
        frag_b(0, 0, 0);
        frag_a(0, 0, 0);
        for (int blk = b0; blk < b1; ++blk) {
            const int sl = (blk - b0) & 1;
            frag_b(1, sl, 1);
            frag_a(1, sl, 1);
            mma(0);
            pin(with_b{});
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            __builtin_amdgcn_sched_barrier(0);
            const int nxt = min(blk + 2, last);  // uniform; the tail reloads the last block
            dma_a(nxt, 0, sl);
            dma_b(nxt, sl);
            frag_b(0, sl ^ 1, 0);  // block s + 1 (the tail's extra read is discarded)
            frag_a(0, sl ^ 1, 0);
            mma(1);
            pin(with_b{});
        }
    }
    // the tail's reloads land and every wave's last reads are done before the
    // epilogue reuses the LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    float* out = PARTIAL ? Y + (size_t)blockIdx.y * M * ldy : Y;
    gemm3_store<WM, WN, FI, FJ, PRELU, !PARTIAL, 2 * ASLOT + 2 * BSLOT, PARTS>(acc, lds, lane, wr, wc, m0, n0, M, N, bias,
                                                                               out, ldy, a);
}

// ---------------------------------------------------------------------------
// int8 activations (tcsc_gpu_sgemm_i8).  X8 (M x ld8 bytes) and
// the plan's int8 image of W^T (N x ld8), ld8 = mfma8_ldw(K): rows of whole
// 128-k blocks, zeros past K.  Integers are never non-finite or tiny: no row
// flags, no fixup; the i32 sums are exact, so every K split gives one result.
// ---------------------------------------------------------------------------
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));  // i32x4: tcsc_w2.h

// The epilogue arithmetic, act(fl(fl(fl(float(S) * s) * c) + b)) as floats or
// rounded to bf16, is i8_out and i8_bf16 of tcsc_i8_out.h:
// k_decode8 and k_decode8q (tcsc_decode.hip) run the same definitions.

// int8 X (M x K, pitch K) -> X8 (M x ld8 bytes): the row as it is, zeros past
// K, one workgroup per row.  VEC (K % 16 == 0, X 16-B aligned): kSplitU 16-B
// loads in flight per thread, 16-B stores; otherwise byte by byte.
__global__ void __launch_bounds__(256) k_pack8(const int8_t* __restrict__ X, int M, int K, int8_t* __restrict__ X8,
                                              int ld8) {
    const int row = blockIdx.x;
    const int8_t* src = X + (size_t)row * K;
    int8_t* dst = X8 + (size_t)row * ld8;
    const bool vec = (K & 15) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (vec) {
        const int ko = K / 16;
        for (int q0 = threadIdx.x; q0 < ko; q0 += kSplitU * blockDim.x) {
            u32x4 w[kSplitU];
#pragma unroll
            for (int u = 0; u < kSplitU; ++u) {
                const int q = q0 + u * blockDim.x;
                if (q < ko) w[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + 16 * q));
            }
#pragma unroll
            for (int u = 0; u < kSplitU; ++u) {
                const int q = q0 + u * blockDim.x;
                if (q >= ko) break;
                *reinterpret_cast<u32x4*>(dst + 16 * q) = w[u];
            }
        }
    } else {
        for (int k = threadIdx.x; k < K; k += blockDim.x) dst[k] = src[k];
    }
    for (int i = K + threadIdx.x; i < ld8; i += blockDim.x) dst[i] = 0;
}

// The int8 image from the bf16 one: WT (ncols x ldw bf16, small integers) ->
// W8 (ncols x ld8 bytes, zeros past K), one workgroup per column of W.  *bad =
// 1 when a weight is outside [-127, 127] or a column's sum of |w| reaches 2^24
// (then |sum_k q w| could pass 2^31 for some int8 X).
__global__ void __launch_bounds__(256) k_w8_from(const uint16_t* __restrict__ WT, int ncols, int K, int ldw,
                                                int8_t* __restrict__ W8, int ld8, int* __restrict__ bad) {
    __shared__ unsigned long long tot[256];
    const int j = blockIdx.x;
    const uint16_t* src = WT + (size_t)j * ldw;
    int8_t* dst = W8 + (size_t)j * ld8;
    unsigned long long sum = 0;
    bool wide = false;
    for (int k = threadIdx.x; k < ld8; k += blockDim.x) {
        int w = 0;
        if (k < K) w = (int)u2f((uint32_t)src[k] << 16);
        const int m = w < 0 ? -w : w;
        wide |= m > 127;
        sum += (unsigned long long)m;
        dst[k] = (int8_t)w;
    }
    tot[threadIdx.x] = sum;
    wide = __syncthreads_or(wide);
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) tot[threadIdx.x] += tot[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && (wide || tot[0] >= (1ull << 24))) *bad = 1;
}

// Split K: the i32 slabs added as integers (any order gives the same sum),
// then the unsplit epilogue's arithmetic.  VEC: 4 columns per thread (N % 4 ==
// 0, ldy % 4 == 0, 16-B aligned slabs, Y aligned to 4 of its elements), all
// slices' loads in flight.  TY: float, or uint16_t for a bf16 Y (§21).  GLU (§24):
// the value is the up half of a gated call and Y = i8_glu(G[row, col], value, act);
// VEC then asks 16-B alignment and ldg % 4 == 0 of G too.  RES (§26): what is
// stored is i8_res(value, R[row, col]), R of Y's type at pitch ldr and read by
// the thread that stores the element, ahead of the store (R == Y is allowed, so
// neither carries restrict); VEC then asks R aligned to four elements and
// ldr % 4 == 0 as well.
template <bool PRELU, bool VEC, typename TY, bool GLU = false, bool RES = false>
__global__ void __launch_bounds__(256) k_reduce_i8(const int* __restrict__ ws, int slices, int M, int N,
                                                   const float* __restrict__ scale,
                                                   const float* __restrict__ cscale, const float* __restrict__ Bias,
                                                   I8YPtr<TY, RES> Y, int ldy, float a,
                                                   const float* __restrict__ G = nullptr, int ldg = 0, int act = 0,
                                                   const TY* R = nullptr, int ldr = 0) {
    static_assert(!(GLU && PRELU), "the halves of a gated call have no PReLU");
    static_assert(!(RES && (GLU || PRELU)), "a residual call is neither gated nor has it a PReLU");
    constexpr int W = VEC ? 4 : 1;
    const int nq = N / W;
    const long long total = (long long)M * nq;
    const int nslices = slices;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        // The loop's own copies of the slice count and the slab size.  RES: the empty asm makes them values
        // of this iteration, so the 16 compares `s < slices` and the 15 products s * slab are made where they
        // are used; hoisted out of the loop they are 16 masks and 15 offsets in some 60 SGPRs that live
        // across it, and with R and ldr on top the residual form spilled 6 to 12 SGPRs.  The other forms
        // keep their code (and the spills they had).
        int slices = nslices;
        size_t slab = (size_t)M * N;
        if constexpr (RES) asm volatile("" : "+s"(slices), "+s"(slab));
        const int row = (int)(i / nq), col = W * (int)(i % nq);
        const size_t e = (size_t)row * N + col;
        int p[16][W];
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (s < slices) {
                if constexpr (VEC) {
                    const i32x4 q = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(ws + s * slab + e));
#pragma unroll
                    for (int u = 0; u < 4; ++u) p[s][u] = q[u];
                } else {
                    p[s][0] = ws[s * slab + e];
                }
            }
        const float sc = scale ? scale[row] : 1.0f;
        float v[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
            int t = 0;
#pragma unroll
            for (int s = 0; s < 16; ++s)
                if (s < slices) t += p[s][u];
            v[u] = i8_out<PRELU>(t, sc, i8_cscale(cscale, col + u), Bias[col + u], a);
        }
        if constexpr (GLU) {
            const float* gp = G + (size_t)row * ldg + col;
            if constexpr (VEC) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(gp);
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = i8_glu(g[u], v[u], act);
            } else {
                v[0] = i8_glu(gp[0], v[0], act);
            }
        }
        if constexpr (RES) {
            const TY* rp = R + (size_t)row * ldr + col;
            if constexpr (VEC) {
                float r[4];
                I8Y<TY>::get4(rp, r);
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = i8_res(v[u], r[u]);
            } else {
                v[0] = i8_res(v[0], I8Y<TY>::get(rp));
            }
        }
        TY* dst = Y + (size_t)row * ldy + col;
        if constexpr (VEC)
            I8Y<TY>::put4_nt(dst, v[0], v[1], v[2], v[3]);
        else
            I8Y<TY>::put(dst, v[0]);
    }
}

// The k_gemm8 epilogue: gemm3_store's staging (the raw i32 sums parked in the
// LDS, read back as whole rows, 16-B stores).  PARTIAL: the raw sums go into
// the i32 slab (Yi, pitch ldy); otherwise Y = i8_out(S, scale[row], cscale[col],
// bias[col]), as floats or (TY = uint16_t) bf16 bits.  A lane's four columns go
// out as one store -- 16 B of floats, 8 B of bf16 -- where Y is aligned to four
// of its elements and ldy % 4 == 0, else element by element, each guarded.
// GLU (§24): the value is the up half of a gated call, and what is stored is
// i8_glu(G[row, col], value, act), G the gate half's fp32 output at pitch ldg.
// RES (§26): what is stored is i8_res(value, R[row, col]), R of Y's type at pitch
// ldr.  A lane reads the four columns it stores, ahead of the store -- as one
// load where the store is one and R is aligned to four elements with ldr % 4 ==
// 0 too, else element by element, each guarded -- so R == Y (ldr == ldy) reads
// every element once.  Y carries no restrict here: the kernels' own Y parameter
// does, except in the residual instantiations (I8YPtr).
template <int WM, int WN, int FI, int FJ, bool PRELU, bool PARTIAL, int LDSB, bool GLU = false, bool RES = false,
          typename TY>
__device__ __forceinline__ void gemm8_store(const i32x4 (&acc)[FI][FJ], char* lds, int lane, int wr, int wc, int m0,
                                            int n0, int M, int N, const float* __restrict__ scale,
                                            const float* __restrict__ cscale, const float* __restrict__ bias,
                                            TY* Y, int ldy, float a,
                                            const float* __restrict__ G = nullptr, int ldg = 0, int act = 0,
                                            const TY* R = nullptr, int ldr = 0) {
    static_assert(!PARTIAL || std::is_same<TY, float>::value, "the i32 slabs travel as the float instantiation");
    static_assert(!GLU || (!PARTIAL && !PRELU), "a gated store is a final one, and its halves have no PReLU");
    static_assert(!RES || (!PARTIAL && !PRELU && !GLU), "a residual store is a final one, not gated and without PReLU");
    constexpr int TM = WM * FI * 16, TN = WN * FJ * 16, NW = WM * WN;
    constexpr int PR = 64, SROW = TN + 4, LPR = TN / 4;  // rows per pass, staged row, lanes per row
    static_assert(PR * SROW * 4 <= LDSB && TM % PR == 0 && (64 % LPR == 0 || LPR % 64 == 0), "epilogue staging");
    static_assert((NW * 64) % LPR == 0, "a lane keeps its columns across the read-back");
    int* stg = reinterpret_cast<int*>(lds);
    bool vec = (ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(Y) & (4 * sizeof(TY) - 1)) == 0;
    if constexpr (RES) vec = vec && (ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(R) & (4 * sizeof(TY) - 1)) == 0;
    const int c4 = 4 * (threadIdx.x % LPR), col = n0 + c4;
    f32x4 bq = f32x4{0.f, 0.f, 0.f, 0.f}, cq = f32x4{1.f, 1.f, 1.f, 1.f};
    if (!PARTIAL) {
#pragma unroll
        for (int u = 0; u < 4; ++u) bq[u] = col + u < N ? bias[col + u] : 0.0f;
        if (cscale)
#pragma unroll
            for (int u = 0; u < 4; ++u) cq[u] = col + u < N ? cscale[col + u] : 1.0f;
    }
#pragma unroll
    for (int p = 0; p < TM / PR; ++p) {
#pragma unroll
        for (int i = 0; i < FI; ++i) {
            if (((wr * FI + i) * 16) / PR != p) continue;  // uniform
            const int rb = (wr * FI + i) * 16 - p * PR + 4 * (lane >> 4);
#pragma unroll
            for (int j = 0; j < FJ; ++j) {
                const int c = (wc * FJ + j) * 16 + (lane & 15);
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) stg[(rb + rg) * SROW + c] = acc[i][j][rg];
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < PR * LPR; e += NW * 64) {
            const int r = e / LPR;
            const int row = m0 + p * PR + r;
            if (row >= M) continue;
            const i32x4 s = *reinterpret_cast<const i32x4*>(stg + r * SROW + c4);
            if constexpr (PARTIAL) {
                int* dst = reinterpret_cast<int*>(Y) + (size_t)row * ldy + col;
                if (vec && col + 3 < N) {
                    __builtin_nontemporal_store(s, reinterpret_cast<i32x4*>(dst));
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (col + u < N) __builtin_nontemporal_store(s[u], dst + u);
                }
            } else {
                const float sc = scale ? scale[row] : 1.0f;
                f32x4 v;
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = i8_out<PRELU>(s[u], sc, cq[u], bq[u], a);
                if constexpr (GLU) {
                    const float* gp = G + (size_t)row * ldg + col;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (col + u < N) v[u] = i8_glu(gp[u], v[u], act);
                }
                if constexpr (RES) {
                    const TY* rp = R + (size_t)row * ldr + col;
                    float r[4] = {0.f, 0.f, 0.f, 0.f};
                    if (vec && col + 3 < N) {
                        I8Y<TY>::get4(rp, r);
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (col + u < N) r[u] = I8Y<TY>::get(rp + u);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = i8_res(v[u], r[u]);
                }
                TY* dst = Y + (size_t)row * ldy + col;
                if (vec && col + 3 < N) {
                    I8Y<TY>::put4_nt(dst, v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (col + u < N) I8Y<TY>::put_nt(dst + u, v[u]);
                }
            }
        }
        __syncthreads();  // the staging is reused by the next pass
    }
}

// k_gemm8: k_gemm3's one-part form on int8 (a sibling, so the bf16 kernels'
// code stays what it was).  A sub-step is a 128-k block: the same 128-byte
// rows, 1-KiB pieces, 16-B DMA granules, swizzle, rings and half-step
// pipeline; a lane's 16-B fragment holds 16 int8 for
// v_mfma_i32_16x16x64_i8, two of them (kh 0, 1) per row and sub-step.  A and W
// are read with the same lane -> byte mapping, so both operands hold the same
// k values whichever they are, and an integer dot product does not depend on
// their order.  ldk = ldw = mfma8_ldw(K) bytes.  PARTIAL: raw i32 sums into
// slab blockIdx.y of Y (M x ldy ints), added by k_reduce_i8.
template <int WM, int WN, int FI, int FJ, bool PRELU, bool PARTIAL, typename TY = float, bool RES = false>
__global__ void __launch_bounds__(WM * WN * 64) k_gemm8(const int8_t* __restrict__ A, const int8_t* __restrict__ Bt,
                                                      int ldk, int ldw, int M, int N, int nblk,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ cscale,
                                                      const float* __restrict__ bias, I8YPtr<TY, RES> Y, int ldy,
                                                      float a, int tiles_m, int tiles_n, int gm, int bps,
                                                      const TY* R = nullptr, int ldr = 0) {
    static_assert(!(PARTIAL && PRELU), "a partial slab carries raw sums");
    constexpr int TM = WM * FI * 16, TN = WN * FJ * 16, NW = WM * WN;
    constexpr int PA = TM / 8, PB = TN / 8;  // 1-KiB pieces of a slot
    constexpr int ASLOT = PA * 1024, BSLOT = PB * 1024, BOFF = 2 * ASLOT;
    constexpr int PAW = PA / NW, PBW = PB / NW;  // pieces each wave moves per A / B slot
    static_assert(PA % NW == 0 && PB % NW == 0, "whole pieces per wave");
    __shared__ __attribute__((aligned(1024))) char lds[2 * ASLOT + 2 * BSLOT];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave / WN, wc = wave % WN;

    int m0, n0;
    gemm3_tile<TM, TN>(tiles_m, tiles_n, gm, m0, n0);

    // per-lane byte offsets of this wave's DMA pieces (rows clamped into the matrix)
    const int row_in = lane >> 3, gsel = (lane & 7) ^ row_in;
    uint32_t offa[PAW];
#pragma unroll
    for (int i = 0; i < PAW; ++i)
        offa[i] = (uint32_t)(min(8 * (wave * PAW + i) + row_in, M - 1 - m0) * ldk + 16 * gsel);
    const char* abase = reinterpret_cast<const char*>(A + (size_t)m0 * ldk);
    const char* bbase = reinterpret_cast<const char*>(Bt + (size_t)n0 * ldw);
    auto dma_a = [&](int blk, int slot) {  // X8's 128-k block `blk`
        const char* g = abase + (size_t)kMfma8Blk * blk;
#pragma unroll
        for (int i = 0; i < PAW; ++i)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(g + offa[i]),
                                             (__attribute__((address_space(3))) void*)(lds + slot * ASLOT +
                                                                                       (wave * PAW + i) * 1024),
                                             16, 0, 0);
    };
    auto dma_b = [&](int blk, int slot) {  // W8's 128-k block `blk` (offsets recomputed, as k_gemm3 does)
        const char* g = bbase + (size_t)kMfma8Blk * blk;
#pragma unroll
        for (int i = 0; i < PBW; ++i)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(
                                                 g + (uint32_t)(min(8 * (wave * PBW + i) + row_in, N - 1 - n0) * ldw +
                                                                16 * gsel)),
                                             (__attribute__((address_space(3))) void*)(lds + BOFF + slot * BSLOT +
                                                                                       (wave * PBW + i) * 1024),
                                             16, 0, 0);
    };

    // fragment read offsets inside a 16-row block (k_gemm3's swizzle)
    int foff[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
        foff[kh] = ((lane & 15) >> 3) * 1024 + 16 * (8 * (lane & 7) + ((4 * kh + (lane >> 4)) ^ (lane & 7)));

    i32x4 acc[FI][FJ];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

    i32x4 af[2][FI], bfr[2][FJ];
    auto frag_a = [&](int set, int aslot, int kh) {
        const char* sa = lds + aslot * ASLOT;
#pragma unroll
        for (int i = 0; i < FI; ++i)
            af[set][i] = *reinterpret_cast<const i32x4*>(sa + ((wr * FI + i) * 2) * 1024 + foff[kh]);
    };
    auto frag_b = [&](int set, int bslot, int kh) {
        const char* sb = lds + BOFF + bslot * BSLOT;
#pragma unroll
        for (int j = 0; j < FJ; ++j)
            bfr[set][j] = *reinterpret_cast<const i32x4*>(sb + ((wc * FJ + j) * 2) * 1024 + foff[kh]);
    };
    auto mma = [&](int set) {
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
            for (int j = 0; j < FJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[set][i], bfr[set][j], acc[i][j], 0, 0, 0);
    };

    // the half steps pinned as in k_gemm3: one read per MFMA pair
    constexpr int NM = FI * FJ, NR = FI + FJ;
    static_assert(2 * NR <= NM, "one read per MFMA pair");
    auto pin = [&]() {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
        }
        if constexpr (NM > 2 * NR) __builtin_amdgcn_sched_group_barrier(0x008, NM - 2 * NR, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    // this workgroup's 128-k blocks (the host makes every slice non-empty)
    const int b0 = PARTIAL ? (int)blockIdx.y * bps : 0;
    const int b1 = PARTIAL ? min(nblk, b0 + bps) : nblk;
    const int last = b1 - 1;
    dma_a(b0, 0);
    dma_b(b0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    dma_a(min(b0 + 1, last), 1);
    dma_b(min(b0 + 1, last), 1);
    frag_b(0, 0, 0);
    frag_a(0, 0, 0);
    for (int blk = b0; blk < b1; ++blk) {
        const int sl = (blk - b0) & 1;
        frag_b(1, sl, 1);
        frag_a(1, sl, 1);
        mma(0);
        pin();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        const int nxt = min(blk + 2, last);  // uniform; the tail reloads the last block
        dma_a(nxt, sl);
        dma_b(nxt, sl);
        frag_b(0, sl ^ 1, 0);  // block s + 1 (the tail's extra read is discarded)
        frag_a(0, sl ^ 1, 0);
        mma(1);
        pin();
    }
    // the tail's reloads land and every wave's last reads are done before the
    // epilogue reuses the LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    TY* out = PARTIAL ? reinterpret_cast<TY*>(reinterpret_cast<int*>(Y) + (size_t)blockIdx.y * M * ldy) : Y;
    gemm8_store<WM, WN, FI, FJ, PRELU, PARTIAL, 2 * ASLOT + 2 * BSLOT, false, RES>(acc, lds, lane, wr, wc, m0, n0, M, N, scale,
                                                                                   cscale, bias, out, ldy, a, nullptr, 0, 0,
                                                                                   R, ldr);
}

// k_gemm8w2: k_gemm8 with the B operand read from the 2-bit
// image of W (tcsc_internal.h, "int8 decode path") instead of the int8 one.
// Only shapes of one wave row (WM = 1): every wave owns its FJ column tiles
// privately, so B never passes through the LDS.  The image is fragment-major:
// the 8 bytes at 16 lane + 8 (blk & 1) of tile (t, blk >> 1) are this lane's two
// B fragments of the 128-k block blk (dword kh = half kh), with the lane -> k
// map of the A fragments.  They are loaded straight into VGPRs two blocks
// ahead, at the point where k_gemm8 issues its B DMA, and expanded in
// registers: int8 dword d is (p >> 2d) & 0x03030303, and the codes c = w + 1
// become signed bytes by one v_perm_b32 that takes each code as the selector
// into the bytes ff, 00, 01 (codes 0, 1, 2 -> -1, 0, +1: a shift, a mask and
// a permute per dword, four fewer VALU per fragment than the arithmetic form
// ((c | 0x80..) - 0x01..) ^ 0x80..), so the MFMAs give S = sum q w itself: no
// row sums, nothing to correct under split K, and the padding code 1 is a
// weight 0.  A (X8), its DMA ring, the swizzle, the half-step pipeline and the
// epilogue are k_gemm8's.  A workgroup's column tiles past the matrix read the
// last tile again and are not stored; an odd count of 128-k blocks ends the
// loop inside the last 256-k image block, whose second half is never read.
template <int WN, int FI, int FJ, bool PRELU, bool PARTIAL, int BS = 2, typename TY = float, bool GLU = false,
          bool RES = false>
__global__ void __launch_bounds__(WN * 64) k_gemm8w2(const int8_t* __restrict__ A, const uint32_t* __restrict__ W2,
                                                    int ldk, int M, int N, int nblk, int nkb, int ntiles,
                                                    const float* __restrict__ scale, const float* __restrict__ cscale,
                                                    const float* __restrict__ bias, I8YPtr<TY, RES> Y, int ldy,
                                                    float a, int tiles_m, int tiles_n, int gm, int bps,
                                                    const float* __restrict__ G = nullptr, int ldg = 0, int act = 0,
                                                    const TY* R = nullptr, int ldr = 0) {
    static_assert(!(PARTIAL && PRELU), "a partial slab carries raw sums");
    constexpr int TM = FI * 16, TN = WN * FJ * 16, NW = WN;
    constexpr int PA = TM / 8, ASLOT = PA * 1024, PAW = PA / NW;
    static_assert(PA % NW == 0, "whole pieces per wave");
    // the A ring, or the epilogue's staging (64 rows of TN + 4 ints) where that is larger
    constexpr int STG = 64 * (TN + 4) * 4, LDSB = 2 * ASLOT > STG ? 2 * ASLOT : STG;
    __shared__ __attribute__((aligned(1024))) char lds[LDSB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    int m0, n0;
    gemm3_tile<TM, TN>(tiles_m, tiles_n, gm, m0, n0);

    const int row_in = lane >> 3, gsel = (lane & 7) ^ row_in;
    uint32_t offa[PAW];
#pragma unroll
    for (int i = 0; i < PAW; ++i)
        offa[i] = (uint32_t)(min(8 * (wave * PAW + i) + row_in, M - 1 - m0) * ldk + 16 * gsel);
    const char* abase = reinterpret_cast<const char*>(A + (size_t)m0 * ldk);
    auto dma_a = [&](int blk, int slot) {
        const char* g = abase + (size_t)kMfma8Blk * blk;
#pragma unroll
        for (int i = 0; i < PAW; ++i)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(g + offa[i]),
                                             (__attribute__((address_space(3))) void*)(lds + slot * ASLOT +
                                                                                       (wave * PAW + i) * 1024),
                                             16, 0, 0);
    };
    // this wave's column tiles, clamped into the image: a uniform base and uniform tile offsets (a column tile is
    // nkb KiB, below 2^24 bytes), so a lane adds only its own 16 lane
    const int tile0 = min(n0 / kW2Cols + wave * FJ, ntiles - 1);
    const char* wbase = reinterpret_cast<const char*>(W2) + (size_t)tile0 * nkb * kW2TileBytes;
    uint32_t toff[FJ];
#pragma unroll
    for (int j = 0; j < FJ; ++j) toff[j] = (uint32_t)(min(tile0 + j, ntiles - 1) - tile0) * nkb * kW2TileBytes;
    auto load_b = [&](int blk, u32x2 (&q)[FJ]) {  // blk < nblk, so blk >> 1 < nkb
        const uint32_t boff = (uint32_t)(blk >> 1) * kW2TileBytes + 8 * (blk & 1);
#pragma unroll
        for (int j = 0; j < FJ; ++j) q[j] = *reinterpret_cast<const u32x2*>(wbase + (toff[j] + boff) + 16 * lane);
    };

    int foff[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
        foff[kh] = ((lane & 15) >> 3) * 1024 + 16 * (8 * (lane & 7) + ((4 * kh + (lane >> 4)) ^ (lane & 7)));

    i32x4 acc[FI][FJ];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

    // BS = 2: the expanded fragments of the two half steps in sets of their own, as the A fragments; BS = 1 (the
    // 8-wave shape, whose two waves per SIMD leave 256 registers each): one set, expanded between the MFMA groups
    static_assert(BS == 1 || BS == 2, "one or two sets of B fragments");
    i32x4 af[2][FI], bfr[BS][FJ];
    // The image dwords of two consecutive 128-k blocks, ping-pong: a round reads the second dword of its own
    // block, then loads the block after next into the same registers, so nothing is copied from round to round.
    // These are ordinary loads that the compiler counts, and it cannot see the explicit waits below: with a
    // register rotation in the loop it waited for each block's loads right after issuing them, and it sank the
    // prologue's loads behind the first barrier.  landed() takes the registers just ahead of the first wait,
    // which keeps the prologue's loads in front of it.
    u32x2 qa[FJ], qb[FJ];
    auto landed = [&](u32x2 (&v)[FJ]) {
#pragma unroll
        for (int j = 0; j < FJ; ++j) asm volatile("" : "+v"(v[j]));
    };
    auto frag_a = [&](int set, int aslot, int kh) {
        const char* sa = lds + aslot * ASLOT;
#pragma unroll
        for (int i = 0; i < FI; ++i) af[set][i] = *reinterpret_cast<const i32x4*>(sa + (i * 2) * 1024 + foff[kh]);
    };
    auto frag_b = [&](int set, const u32x2 (&q)[FJ], int kh) {
#pragma unroll
        for (int j = 0; j < FJ; ++j) bfr[set % BS][j] = w2_frag(q[j][kh]);
    };
    auto mma = [&](int set) {
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
            for (int j = 0; j < FJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[set][i], bfr[set % BS][j], acc[i][j], 0, 0, 0);
    };
    // one A read per MFMA pair, as k_gemm8 pins them; the expansion's VALU is left to the scheduler
    constexpr int NM = FI * FJ, NR = FI;
    static_assert(2 * NR <= NM, "one read per MFMA pair");
    auto pin = [&]() {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
        }
        if constexpr (NM > 2 * NR) __builtin_amdgcn_sched_group_barrier(0x008, NM - 2 * NR, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    // this workgroup's 128-k blocks (the host makes every slice non-empty)
    const int b0 = PARTIAL ? (int)blockIdx.y * bps : 0;
    const int b1 = PARTIAL ? min(nblk, b0 + bps) : nblk;
    const int last = b1 - 1;
    dma_a(b0, 0);
    load_b(b0, qa);
    load_b(min(b0 + 1, last), qb);
    landed(qa);
    landed(qb);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    dma_a(min(b0 + 1, last), 1);
    frag_b(0, qa, 0);
    frag_a(0, 0, 0);
    // one 128-k block: qc holds its image dwords, qn the next block's; sl is its A slot
    auto round = [&](int blk, int sl, u32x2 (&qc)[FJ], const u32x2 (&qn)[FJ]) {
        if constexpr (BS == 2) frag_b(1, qc, 1);
        frag_a(1, sl, 1);
        mma(0);
        pin();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        const int nxt = min(blk + 2, last);  // uniform; the tail reloads the last block
        dma_a(nxt, sl);
        if constexpr (BS == 1) frag_b(1, qc, 1);  // the one set is free once mma(0) is issued
        load_b(nxt, qc);
        if constexpr (BS == 2) frag_b(0, qn, 0);  // block blk + 1 (the tail's extra fragments are discarded)
        frag_a(0, sl ^ 1, 0);
        mma(1);
        pin();
        if constexpr (BS == 1) frag_b(0, qn, 0);
    };
    int blk = b0;
    for (; blk + 1 < b1; blk += 2) {
        round(blk, 0, qa, qb);
        round(blk + 1, 1, qb, qa);
    }
    if (blk < b1) round(blk, 0, qa, qb);  // an odd count of blocks (uniform)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    TY* out = PARTIAL ? reinterpret_cast<TY*>(reinterpret_cast<int*>(Y) + (size_t)blockIdx.y * M * ldy) : Y;
    gemm8_store<1, WN, FI, FJ, PRELU, PARTIAL, LDSB, GLU, RES>(acc, lds, lane, 0, wave, m0, n0, M, N, scale, cscale, bias,
                                                               out, ldy, a, G, ldg, act, R, ldr);
}

// tcsc_gpu_quantize_rows_i8{,_bf16}: per row, amax = max |x|, scale = amax /
// 127, inv = 127 / amax, q = clamp(rint(x * inv), -127, 127); amax = 0, or so
// small that 127 / amax is inf: q = 0, scale = 0 (quant_scales and quant_i8, tcsc_quant.h).  Every step is one
// correctly rounded fp32 operation; TX = uint16_t is bf16 bit patterns, widened
// first (XSrc, exact).  One workgroup per row, the row read twice (the second
// time from the L2).  VEC (K a multiple of the kVec elements of a 16-B load, X
// 16-B and Xq kVec-B aligned): 16-B loads, stores of kVec q.
//
// NORM (tcsc_gpu_quantize_rows_i8_norm): the quantizer of
// xn = RMSNorm(x) gamma.  Three passes -- the sum of squares in tcsc_norm.h's
// order (thread t owns the partials t and t + 256: the groups t + 256 j), the
// maximum of |xn|, the quantized values -- of which only the first reads the
// row where it is short: a thread keeps its first kNormCached groups in
// registers (rows of up to 8192 elements whole), turns them into xn in place
// and quantizes them from there; the groups of a longer row beyond those are
// streamed again in each pass.  VEC then also asks gamma (if any) to be 16-B
// aligned; the q of a half group go out as one 4-B store.  The instantiations
// without NORM are the kernel as it was and read neither gamma nor eps.
constexpr int kNormCached = 4;
template <typename TX, bool VEC, bool NORM = false>
__global__ void __launch_bounds__(256) k_quant_rows_i8(const TX* __restrict__ X, int M, int K,
                                                      int8_t* __restrict__ Xq, float* __restrict__ scale,
                                                      const float* __restrict__ gamma = nullptr, float eps = 0.0f) {
    using XS = XSrc<TX>;
    constexpr int kVec = XS::kVec;
    __shared__ float red[256];
    const int row = blockIdx.x;
    const TX* src = X + (size_t)row * K;
    int8_t* dst = Xq + (size_t)row * K;
    if constexpr (NORM) {
        const int t = threadIdx.x, ngroups = (K + kNormGroup - 1) / kNormGroup;
        constexpr int kStream = 256 * kNormCached;  // the first streamed group of thread 0
        float xc[kNormCached][kNormGroup];
        float p[2] = {0.0f, 0.0f};  // the partials t and t + 256
#pragma unroll
        for (int j = 0; j < kNormCached; ++j) {
            norm_load_group<TX, VEC>(src, K, min(t + 256 * j, ngroups), xc[j]);  // group `ngroups` is past K: zeros, no load
#pragma unroll
            for (int e = 0; e < kNormGroup; ++e) p[j & 1] = norm_sq_add(p[j & 1], xc[j][e]);
        }
        for (int g = kStream + t; g < ngroups; g += 512) {  // two groups a round: partial t, then t + 256
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float x[kNormGroup];
                norm_load_group<TX, VEC>(src, K, min(g + 256 * h, ngroups), x);
#pragma unroll
                for (int e = 0; e < kNormGroup; ++e) p[h] = norm_sq_add(p[h], x[e]);
            }
        }
        const float r = norm_rinv(norm_ss_team<256>(norm_add(p[0], p[1]), red, t), K, eps);
        __syncthreads();  // red is written again below
        float amax = 0.0f;
#pragma unroll
        for (int j = 0; j < kNormCached; ++j) {
            norm_group_xn<VEC>(xc[j], r, gamma, K, min(t + 256 * j, ngroups));
#pragma unroll
            for (int e = 0; e < kNormGroup; ++e) amax = fmaxf(amax, fabsf(xc[j][e]));
        }
        for (int g = kStream + t; g < ngroups; g += 256) {
            float x[kNormGroup];
            norm_load_group<TX, VEC>(src, K, g, x);
            norm_group_xn<VEC>(x, r, gamma, K, g);
#pragma unroll
            for (int e = 0; e < kNormGroup; ++e) amax = fmaxf(amax, fabsf(x[e]));
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));  // fmaxf is exact in any order
        if ((t & 63) == 0) red[t >> 6] = amax;
        __syncthreads();
        float sc, inv;
        quant_scales(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), sc, inv);
        if (t == 0) scale[row] = sc;
        // the q of group g: bytes in memory order, stored where k < K
        auto store_group = [&](int g, const float (&x)[kNormGroup]) {
            const int k0 = kNormGroup * g;
            if constexpr (VEC) {  // K % 4 == 0 and Xq 4-B aligned: a half group is one store or lies past K
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (k0 + 4 * h >= K) break;
                    uint32_t o = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) o |= ((uint32_t)quant_i8(x[4 * h + u], inv) & 0xffu) << (8 * u);
                    *reinterpret_cast<uint32_t*>(dst + k0 + 4 * h) = o;
                }
            } else {
#pragma unroll
                for (int e = 0; e < kNormGroup; ++e)
                    if (k0 + e < K) dst[k0 + e] = (int8_t)quant_i8(x[e], inv);
            }
        };
#pragma unroll
        for (int j = 0; j < kNormCached; ++j)
            if (t + 256 * j < ngroups) store_group(t + 256 * j, xc[j]);
        for (int g = kStream + t; g < ngroups; g += 256) {
            float x[kNormGroup];
            norm_load_group<TX, VEC>(src, K, g, x);
            norm_group_xn<VEC>(x, r, gamma, K, g);
            store_group(g, x);
        }
    } else {
        float amax = 0.0f;
        if (VEC) {
            for (int q = threadIdx.x; q < K / kVec; q += blockDim.x) {
                float w[kVec];
                XS::unpack(*reinterpret_cast<const uint4*>(src + kVec * q), 1.0f, w);
#pragma unroll
                for (int u = 0; u < kVec; ++u) amax = fmaxf(amax, fabsf(w[u]));
            }
        } else {
            for (int k = threadIdx.x; k < K; k += blockDim.x) amax = fmaxf(amax, fabsf(XS::conv(src[k], 1.0f)));
        }
        red[threadIdx.x] = amax;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
            __syncthreads();
        }
        float sc, inv;
        quant_scales(red[0], sc, inv);
        if (threadIdx.x == 0) scale[row] = sc;
        if (VEC) {
            for (int q = threadIdx.x; q < K / kVec; q += blockDim.x) {
                float w[kVec];
                XS::unpack(*reinterpret_cast<const uint4*>(src + kVec * q), 1.0f, w);
                uint32_t o[kVec / 4];
#pragma unroll
                for (int d = 0; d < kVec / 4; ++d) {
                    o[d] = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) o[d] |= ((uint32_t)quant_i8(w[4 * d + u], inv) & 0xffu) << (8 * u);
                }
                if constexpr (kVec == 4)
                    *reinterpret_cast<uint32_t*>(dst + kVec * q) = o[0];
                else
                    *reinterpret_cast<uint2*>(dst + kVec * q) = make_uint2(o[0], o[1]);
            }
        } else {
            for (int k = threadIdx.x; k < K; k += blockDim.x) dst[k] = (int8_t)quant_i8(XS::conv(src[k], 1.0f), inv);
        }
    }
}

// tcsc_gpu_rmsnorm_rows: Xn = fl(fl(x r) gamma) in fp32 and,
// where rinv is given, r per row -- the arithmetic of tcsc_norm.h, one
// workgroup per row, the row read twice.  It is the definition the fused forms
// (k_quant_rows_i8<.., NORM>, k_decode8q<.., NORM>) are compared against.  VEC:
// X as in k_quant_rows_i8, and Xn and gamma (if any) 16-B aligned.
template <typename TX, bool VEC>
__global__ void __launch_bounds__(256) k_rmsnorm_rows(const TX* __restrict__ X, const float* __restrict__ gamma,
                                                     float eps, int M, int K, float* __restrict__ Xn,
                                                     float* __restrict__ rinv) {
    using XS = XSrc<TX>;
    constexpr int kVec = XS::kVec;
    __shared__ float part[256];
    const int row = blockIdx.x;
    const TX* src = X + (size_t)row * K;
    float* dst = Xn + (size_t)row * K;
    const float r =
        norm_rinv(norm_ss_team<256>(norm_ss_thread<TX, 256, VEC>(src, K, threadIdx.x), part, threadIdx.x), K, eps);
    if (threadIdx.x == 0 && rinv) rinv[row] = r;
    if (VEC) {
        for (int q = threadIdx.x; q < K / kVec; q += blockDim.x) {
            float w[kVec];
            XS::unpack(*reinterpret_cast<const uint4*>(src + kVec * q), 1.0f, w);
            norm_piece<kVec>(w, r, gamma, kVec * q);
#pragma unroll
            for (int d = 0; d < kVec / 4; ++d)
                *reinterpret_cast<float4*>(dst + kVec * q + 4 * d) =
                    make_float4(w[4 * d], w[4 * d + 1], w[4 * d + 2], w[4 * d + 3]);
        }
    } else {
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            const float x = XS::conv(src[k], 1.0f);
            dst[k] = gamma ? norm_apply(x, r, gamma[k]) : norm_apply(x, r);
        }
    }
}

}  // namespace

hipError_t csc_prepare(const int* csp, const int* csn, const int* rip, const int* rin, int col_begin, int ncols,
                       long long n_pos, long long n_neg, int* cp, int* cn, int* crp, int* crn, int* gq, void* scan_tmp,
                       size_t scan_tmp_bytes, int* cq, hipStream_t st) {
    hipError_t e;
    if ((e = rebase_offsets(csp, col_begin, ncols, cp, st)) != hipSuccess) return e;
    if ((e = rebase_offsets(csn, col_begin, ncols, cn, st)) != hipSuccess) return e;
    if (n_pos > 0)
        hipLaunchKernelGGL(k_copy_from, dim3(grid_of(n_pos, 256)), dim3(256), 0, st, rip, csp, col_begin, n_pos, crp);
    if (n_neg > 0)
        hipLaunchKernelGGL(k_copy_from, dim3(grid_of(n_neg, 256)), dim3(256), 0, st, rin, csn, col_begin, n_neg, crn);
    const int ng = csc_groups(ncols);
    hipLaunchKernelGGL(k_group_quads, dim3(grid_of((long long)ng + 1, 256)), dim3(256), 0, st, cp, cn, ncols, gq);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return exclusive_scan_i32(gq, cq, ng + 1, scan_tmp, scan_tmp_bytes, st);
}

hipError_t csc_fill(const int* cp, const int* cn, const int* crp, const int* crn, const int* cq, int ncols, int rows,
                    int* crq, size_t crq_entries, hipStream_t st) {
    hipError_t e;
    // the guard quads (and nothing else) stay 0: row 0, read only by the look-ahead
    if ((e = hipMemsetAsync(crq, 0, crq_entries * sizeof(int), st)) != hipSuccess) return e;
    if (ncols > 0)
        hipLaunchKernelGGL(k_merge_csc, dim3(grid_of(ncols, 256)), dim3(256), 0, st, cp, cn, crp, crn, cq, ncols, rows,
                           crq);
    return hipGetLastError();
}

hipError_t mfma_build_wt(const int* csp, const int* csn, const int* rip, const int* rin, int col_begin, int rows,
                         int ncols, float* wf, uint16_t* wt, int ldw, long long n_pos, long long n_neg, int* bad,
                         hipStream_t st) {
    const long long n = (long long)rows * ncols;
    hipError_t e = hipMemsetAsync(wf, 0, (size_t)n * sizeof(float), st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(wt, 0, (size_t)ncols * ldw * sizeof(uint16_t), st)) != hipSuccess) return e;
    const int wpb = 4;  // waves (columns) per block
    if (n_pos > 0)
        hipLaunchKernelGGL(k_w_scatter, dim3((ncols + wpb - 1) / wpb), dim3(64 * wpb), 0, st, csp, rip, col_begin,
                           ncols, rows, 1.0f, wf);
    if (n_neg > 0)
        hipLaunchKernelGGL(k_w_scatter, dim3((ncols + wpb - 1) / wpb), dim3(64 * wpb), 0, st, csn, rin, col_begin,
                           ncols, rows, -1.0f, wf);
    hipLaunchKernelGGL(k_wt_from, dim3(grid_of(n, 256)), dim3(256), 0, st, wf, ncols, rows, wt, ldw, bad);
    return hipGetLastError();
}

hipError_t mfma_split_x(const float* X, int M, int K, uint16_t* x3, int ldk, int* flags, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_split3, dim3(M), dim3(256), 0, st, X, M, K, x3, ldk, flags);
    return hipGetLastError();
}

hipError_t mfma_pack_x(const uint16_t* X, int M, int K, uint16_t* x1, int ldw, int* flags, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack1, dim3(M), dim3(256), 0, st, X, M, K, x1, ldw, flags);
    return hipGetLastError();
}

// Tile choice: 128 x 512 (8 waves) unless a grid of 256 x 256 tiles would
// leave more than half of the 256 CUs idle, then 128 x 128 (4 waves).
bool mfma_big_tiles(int M, int N) { return (long long)((M + 255) / 256) * ((N + 255) / 256) >= 128; }

// M <= 64 on a small grid: 64 x 256 tiles of 4 waves (1 x 4, 64 x 64 each),
// so no MFMA work and no A staging go to rows past M (the 128 x 128 tiles
// would spend half of both on copies of row M - 1).
bool mfma_narrow_tiles(int M, int N) { return M <= 64 && !mfma_big_tiles(M, N); }

// Workgroups of the unsplit grid: 128 x 512 tiles, 64 x 256 or 128 x 128.
long long mfma_tiles(int M, int N) {
    if (mfma_big_tiles(M, N)) return (long long)((M + 127) / 128) * ((N + 511) / 512);
    if (mfma_narrow_tiles(M, N)) return (long long)((M + 63) / 64) * ((N + 255) / 256);
    return (long long)((M + 127) / 128) * ((N + 127) / 128);
}

// Split-K of a grid with fewer tiles than it can run at once: enough slices
// of the 64-k blocks to bring it to ~512 workgroups of the small or narrow
// tiles (two fit a CU: 64 / 80 KiB of LDS, 4 waves each; ~1,024 of the
// narrow ones, whose slices are cheap to reduce: M <= 64) or ~256 of the
// large ones (one per CU), each slice at least 8 blocks, at most 16 slices (k_reduce4's limit);
// normalized so no slice is empty.  Measured (tools/crossover.py, K = N =
// 8192): M = 64 0.199 -> 0.062 ms, M = 256 0.212 -> 0.108, M = 1024 (large
// tiles, 2 slices) 0.456 -> 0.32; targets of 768 / 1024 small tiles or 512
// large ones were slower.  Narrow tiles: 1024 equals 512 at K = N = 8192 (16
// slices either way) and is 19 % faster at M = 16, K = N = 16384.  $TCSC_MFMA_WGS overrides the target (A/B; 0 =
// never split).
int mfma_split_target(bool big, bool narrow) {
    const char* e = std::getenv("TCSC_MFMA_WGS");
    return e ? std::atoi(e) : big ? 256 : narrow ? 1024 : 512;
}

// The rule for a K of nblk blocks: a slice at least min_blk blocks, at most cap slices.
static int split_k(int M, int N, int nblk, int min_blk, int cap) {
    if (M <= 0 || N <= 0) return 1;
    const long long tiles = mfma_tiles(M, N);
    const long long s = std::min<long long>(
        {mfma_split_target(mfma_big_tiles(M, N), mfma_narrow_tiles(M, N)) / tiles, cap, nblk / min_blk});
    if (s < 2) return 1;
    const int bps = (int)((nblk + s - 1) / s);
    return (nblk + bps - 1) / bps;
}

int mfma_slices(int M, int N, int K) { return split_k(M, N, mfma_nblk(K), 8, 16); }

size_t mfma_slab_bytes(int M, int N, int K) {
    const int s = mfma_slices(M, N, K);
    return s > 1 ? (size_t)s * M * N * sizeof(float) : 0;
}

template <bool PRELU, int PARTS>
static hipError_t launch_gemm3_t(const uint16_t* x3, int ldk, const uint16_t* wt, int ldw, int K, int nblk, int M,
                                 int N, const float* B, float* Y, int ldy, float a, float* slabs, int slices,
                                 const int* flags, const int* cq, const int* crq, hipStream_t st) {
    // bands of 4 row tiles: an XCD's 32 workgroups share 4 A tiles (staged every
    // sub-step) and 8 W tiles (once per block); 8 x 4 was 2 % slower at cfg 5
    constexpr int kGm = 4;
    if (mfma_big_tiles(M, N)) {
        // 128 x 512 tiles of 8 waves (1 x 8, 128 x 64 each): A, staged every
        // sub-step, is the narrow side (37.3 KiB staged per sub-step, 256 x 256
        // tiles: 42.7; 1.4 % faster at cfg 5).  Its LDS is the whole 160 KiB.
        const int tm = (M + 127) / 128, tn = (N + 511) / 512;
        const int gm = std::min(kGm, tm);
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm3<1, 8, 8, 4, PRELU, false, PARTS>), dim3(tm * tn), dim3(512), 0, st, x3, wt, ldk, ldw,
                               M, N, nblk, B, Y, ldy, a, tm, tn, gm, nblk);
        else
            hipLaunchKernelGGL((k_gemm3<1, 8, 8, 4, false, true, PARTS>), dim3(tm * tn, slices), dim3(512), 0, st, x3, wt,
                               ldk, ldw, M, N, nblk, nullptr, slabs, N, 0.0f, tm, tn, gm, (nblk + slices - 1) / slices);
    } else if (mfma_narrow_tiles(M, N)) {
        const int tn = (N + 255) / 256;
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm3<1, 4, 4, 4, PRELU, false, PARTS>), dim3(tn), dim3(256), 0, st, x3, wt, ldk, ldw, M, N,
                               nblk, B, Y, ldy, a, 1, tn, 1, nblk);
        else
            hipLaunchKernelGGL((k_gemm3<1, 4, 4, 4, false, true, PARTS>), dim3(tn, slices), dim3(256), 0, st, x3, wt, ldk, ldw,
                               M, N, nblk, nullptr, slabs, N, 0.0f, 1, tn, 1, (nblk + slices - 1) / slices);
    } else {
        const int tm = (M + 127) / 128, tn = (N + 127) / 128;
        const int gm = std::min(kGm, tm);
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm3<2, 2, 4, 4, PRELU, false, PARTS>), dim3(tm * tn), dim3(256), 0, st, x3, wt, ldk, ldw,
                               M, N, nblk, B, Y, ldy, a, tm, tn, gm, nblk);
        else
            hipLaunchKernelGGL((k_gemm3<2, 2, 4, 4, false, true, PARTS>), dim3(tm * tn, slices), dim3(256), 0, st, x3, wt,
                               ldk, ldw, M, N, nblk, nullptr, slabs, N, 0.0f, tm, tn, gm, (nblk + slices - 1) / slices);
    }
    // split K: raw partial tiles went into slabs[slice] (M x N); then
    // act(s0 + s1 + ... + b) in slice order, flagged rows exact (k_fixup's)
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices <= 1) return e;
    const bool vec = N % 4 == 0 && ldy % 4 == 0 &&
                     ((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(slabs) |
                       reinterpret_cast<uintptr_t>(B)) & 15) == 0;
    const long long n = (long long)M * (vec ? N / 4 : N);
    if (vec)
        hipLaunchKernelGGL((k_reduce_fix<PRELU, true, PARTS>), dim3(grid_of(n, 256)), dim3(256), 0, st, slabs, slices, M, N, B,
                           Y, ldy, a, flags, x3, K, ldk, cq, crq);
    else
        hipLaunchKernelGGL((k_reduce_fix<PRELU, false, PARTS>), dim3(grid_of(n, 256)), dim3(256), 0, st, slabs, slices, M, N,
                           B, Y, ldy, a, flags, x3, K, ldk, cq, crq);
    return hipGetLastError();
}

template <int PARTS>
static hipError_t gemm_parts(const uint16_t* xp, int ldk, const uint16_t* wt, int ldw, int K, int M, int N,
                             const float* B, float* Y, int ldy, bool prelu, float a, float* slabs, size_t slab_bytes,
                             const int* flags, const int* cq, const int* crq, hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    const int nblk = mfma_nblk(K);
    if (nblk < 1 || ldk != (PARTS == 3 ? mfma_ldk(K) : mfma_ldw(K)) || ldw != mfma_ldw(K)) return hipErrorInvalidValue;
    const int slices = mfma_slices(M, N, K);
    if (slices > 1 && (!slabs || slab_bytes < mfma_slab_bytes(M, N, K))) return hipErrorInvalidValue;
    return prelu ? launch_gemm3_t<true, PARTS>(xp, ldk, wt, ldw, K, nblk, M, N, B, Y, ldy, a, slabs, slices, flags, cq,
                                               crq, st)
                 : launch_gemm3_t<false, PARTS>(xp, ldk, wt, ldw, K, nblk, M, N, B, Y, ldy, a, slabs, slices, flags,
                                                cq, crq, st);
}

hipError_t mfma_gemm3(const uint16_t* x3, int ldk, const uint16_t* wt, int ldw, int K, int M, int N, const float* B,
                      float* Y, int ldy, bool prelu, float a, float* slabs, size_t slab_bytes, const int* flags,
                      const int* cq, const int* crq, hipStream_t st) {
    return gemm_parts<3>(x3, ldk, wt, ldw, K, M, N, B, Y, ldy, prelu, a, slabs, slab_bytes, flags, cq, crq, st);
}

hipError_t mfma_gemm1(const uint16_t* x1, int ldk, const uint16_t* wt, int ldw, int K, int M, int N, const float* B,
                      float* Y, int ldy, bool prelu, float a, float* slabs, size_t slab_bytes, const int* flags,
                      const int* cq, const int* crq, hipStream_t st) {
    return gemm_parts<1>(x1, ldk, wt, ldw, K, M, N, B, Y, ldy, prelu, a, slabs, slab_bytes, flags, cq, crq, st);
}

template <int PARTS>
static hipError_t fixup_parts(const uint16_t* xp, int M, int K, int ldk, const int* cq, const int* crq, int ncols,
                              const float* B, float* Y, int ldy, bool bias_first, bool prelu, float a,
                              const int* flags, hipStream_t st) {
    const dim3 grid((ncols + 255) / 256), block(256);
#define TCSC_FIX_ARGS xp, M, K, ldk, cq, crq, ncols, B, Y, ldy, a, flags
    if (bias_first) {
        if (prelu)
            hipLaunchKernelGGL((k_fixup<true, true, PARTS>), grid, block, 0, st, TCSC_FIX_ARGS);
        else
            hipLaunchKernelGGL((k_fixup<true, false, PARTS>), grid, block, 0, st, TCSC_FIX_ARGS);
    } else {
        if (prelu)
            hipLaunchKernelGGL((k_fixup<false, true, PARTS>), grid, block, 0, st, TCSC_FIX_ARGS);
        else
            hipLaunchKernelGGL((k_fixup<false, false, PARTS>), grid, block, 0, st, TCSC_FIX_ARGS);
    }
#undef TCSC_FIX_ARGS
    return hipGetLastError();
}

hipError_t mfma_fixup(const uint16_t* x3, int M, int K, int ldk, const int* cq, const int* crq, int ncols,
                      const float* B, float* Y, int ldy, bool bias_first, bool prelu, float a, const int* flags,
                      hipStream_t st) {
    return fixup_parts<3>(x3, M, K, ldk, cq, crq, ncols, B, Y, ldy, bias_first, prelu, a, flags, st);
}

hipError_t mfma_fixup1(const uint16_t* x1, int M, int K, int ldk, const int* cq, const int* crq, int ncols,
                       const float* B, float* Y, int ldy, bool bias_first, bool prelu, float a, const int* flags,
                       hipStream_t st) {
    return fixup_parts<1>(x1, M, K, ldk, cq, crq, ncols, B, Y, ldy, bias_first, prelu, a, flags, st);
}

// ---- int8 (tcsc_gpu_sgemm_i8) ------------------------------------------------

// mfma_slices' logic counted in 128-k blocks: the same workgroup targets, a
// slice at least 4 blocks (the 512 k of mfma_slices' 8 blocks of 64), and
// never more slices than the fp32 call takes at this shape: the i32 slabs then
// fit the fp32 call's slab space (4 B per element either way), which is what
// keeps the int8 workspace inside the reserved one.
int mfma8_slices(int M, int N, int K) { return split_k(M, N, mfma8_nblk(K), 4, std::min(16, mfma_slices(M, N, K))); }

size_t mfma8_slab_bytes(int M, int N, int K) {
    const int s = mfma8_slices(M, N, K);
    return s > 1 ? (size_t)s * M * N * sizeof(int) : 0;
}

hipError_t mfma8_pack_x(const int8_t* X, int M, int K, int8_t* x8, int ld8, hipStream_t st) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack8, dim3(M), dim3(256), 0, st, X, M, K, x8, ld8);
    return hipGetLastError();
}

hipError_t mfma8_build_w8(const uint16_t* wt, int ncols, int K, int ldw, int8_t* w8, int ld8, int* bad,
                          hipStream_t st) {
    if (ncols <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_w8_from, dim3(ncols), dim3(256), 0, st, wt, ncols, K, ldw, w8, ld8, bad);
    return hipGetLastError();
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

hipError_t quantize_rows_i8(const void* X, int xtype, const RmsNorm* norm, int M, int K, int8_t* Xq, float* scale,
                            hipStream_t st) {
    if (M <= 0) return hipSuccess;
    if (norm && (K < 1 || !X || !Xq || !scale)) return hipErrorInvalidValue;
    return with_elem(xtype == kBf16, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        const TX* x = static_cast<const TX*>(X);
        const bool vec = XSrc<TX>::vec_ok(x, K) && (reinterpret_cast<uintptr_t>(Xq) & (XSrc<TX>::kVec - 1)) == 0 &&
                         (!norm || aligned16(norm->gamma));
        return with_bool(vec, [&](auto v) {
            return with_bool(norm != nullptr, [&](auto nm) {
                hipLaunchKernelGGL((k_quant_rows_i8<TX, decltype(v)::value, decltype(nm)::value>), dim3(M), dim3(256), 0,
                                   st, x, M, K, Xq, scale, norm ? norm->gamma : nullptr, norm ? norm->eps : 0.0f);
                return hipGetLastError();
            });
        });
    });
}

hipError_t rmsnorm_rows(const void* X, bool bf16, const float* gamma, float eps, int M, int K, float* Xn, float* rinv,
                        hipStream_t st) {
    if (M <= 0) return hipSuccess;
    if (K < 1 || !X || !Xn) return hipErrorInvalidValue;
    return with_elem(bf16, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        const TX* x = static_cast<const TX*>(X);
        return with_bool(XSrc<TX>::vec_ok(x, K) && aligned16(Xn) && aligned16(gamma), [&](auto v) {
            hipLaunchKernelGGL((k_rmsnorm_rows<TX, decltype(v)::value>), dim3(M), dim3(256), 0, st, x, gamma, eps, M, K,
                               Xn, rinv);
            return hipGetLastError();
        });
    });
}

// k_reduce_i8 on the slabs of a split int8 GEMM (k_gemm8 or k_gemm8w2)
static hipError_t launch_reduce_i8(const int* slabs, int slices, int M, int N, const I8Epi& e, hipStream_t st) {
    return with_elem(e.y.ytype == kYBf16, [&](auto ty) {
        using TY = typename decltype(ty)::type;
        TY* Y = static_cast<TY*>(e.y.Y);
        const TY* R = static_cast<const TY*>(e.R);
        const bool vec = N % 4 == 0 && e.ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(Y) & (4 * sizeof(TY) - 1)) == 0 &&
                         aligned16(slabs) && (!e.G || (e.ldg % 4 == 0 && aligned16(e.G))) &&
                         (!R || (e.ldr % 4 == 0 && (reinterpret_cast<uintptr_t>(R) & (4 * sizeof(TY) - 1)) == 0));
        const long long n = (long long)M * (vec ? N / 4 : N);
        return with_bool(vec, [&](auto v) {
            if (R) {  // a residual call (never gated, never with a PReLU: mfma8_gemm and mfma8_gemm_w2 refuse both)
                hipLaunchKernelGGL((k_reduce_i8<false, decltype(v)::value, TY, false, true>), dim3(grid_of(n, 256)), dim3(256),
                                   0, st, slabs, slices, M, N, e.rscale, e.y.cscale, e.B, Y, e.ldy, e.a, nullptr, 0, 0, R,
                                   e.ldr);
                return hipGetLastError();
            }
            if (e.G) {  // the up half of a gated call (never with a PReLU: mfma8_gemm_w2 refuses it)
                hipLaunchKernelGGL((k_reduce_i8<false, decltype(v)::value, TY, true>), dim3(grid_of(n, 256)), dim3(256), 0,
                                   st, slabs, slices, M, N, e.rscale, e.y.cscale, e.B, Y, e.ldy, e.a, e.G, e.ldg, e.act);
                return hipGetLastError();
            }
            return with_bool(e.prelu, [&](auto pr) {
                hipLaunchKernelGGL((k_reduce_i8<decltype(pr)::value, decltype(v)::value, TY>), dim3(grid_of(n, 256)),
                                   dim3(256), 0, st, slabs, slices, M, N, e.rscale, e.y.cscale, e.B, Y, e.ldy, e.a);
                return hipGetLastError();
            });
        });
    });
}

template <bool PRELU, typename TY, bool RES = false>
static hipError_t launch_gemm8_t(const int8_t* x8, const int8_t* w8, int ld8, int nblk, int M, int N, const I8Epi& epi,
                                 int* slabs, int slices, hipStream_t st) {
    constexpr int kGm = 4;  // bands of 4 row tiles, as launch_gemm3_t
    const float *scale = epi.rscale, *cscale = epi.y.cscale, *B = epi.B;  // the kernels' parameter lists
    TY* Y = static_cast<TY*>(epi.y.Y);
    const TY* R = static_cast<const TY*>(epi.R);
    const int ldy = epi.ldy;
    const float a = epi.a;
    float* sl = reinterpret_cast<float*>(slabs);
    const int bps = (nblk + slices - 1) / std::max(slices, 1);
    if (mfma_big_tiles(M, N)) {
        const int tm = (M + 127) / 128, tn = (N + 511) / 512;
        const int gm = std::min(kGm, tm);
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm8<1, 8, 8, 4, PRELU, false, TY, RES>), dim3(tm * tn), dim3(512), 0, st, x8, w8, ld8, ld8, M, N,
                               nblk, scale, cscale, B, Y, ldy, a, tm, tn, gm, nblk, R, epi.ldr);
        else
            hipLaunchKernelGGL((k_gemm8<1, 8, 8, 4, false, true>), dim3(tm * tn, slices), dim3(512), 0, st, x8, w8, ld8,
                               ld8, M, N, nblk, nullptr, nullptr, nullptr, sl, N, 0.0f, tm, tn, gm, bps);
    } else if (mfma_narrow_tiles(M, N)) {
        const int tn = (N + 255) / 256;
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm8<1, 4, 4, 4, PRELU, false, TY, RES>), dim3(tn), dim3(256), 0, st, x8, w8, ld8, ld8, M, N, nblk,
                               scale, cscale, B, Y, ldy, a, 1, tn, 1, nblk, R, epi.ldr);
        else
            hipLaunchKernelGGL((k_gemm8<1, 4, 4, 4, false, true>), dim3(tn, slices), dim3(256), 0, st, x8, w8, ld8, ld8, M,
                               N, nblk, nullptr, nullptr, nullptr, sl, N, 0.0f, 1, tn, 1, bps);
    } else {
        const int tm = (M + 127) / 128, tn = (N + 127) / 128;
        const int gm = std::min(kGm, tm);
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm8<2, 2, 4, 4, PRELU, false, TY, RES>), dim3(tm * tn), dim3(256), 0, st, x8, w8, ld8, ld8, M, N,
                               nblk, scale, cscale, B, Y, ldy, a, tm, tn, gm, nblk, R, epi.ldr);
        else
            hipLaunchKernelGGL((k_gemm8<2, 2, 4, 4, false, true>), dim3(tm * tn, slices), dim3(256), 0, st, x8, w8, ld8,
                               ld8, M, N, nblk, nullptr, nullptr, nullptr, sl, N, 0.0f, tm, tn, gm, bps);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices <= 1) return e;
    return launch_reduce_i8(slabs, slices, M, N, epi, st);
}

// k_gemm8w2 on k_gemm8's three grids, slices and blocks per slice: 128 x 512
// (8 waves of 128 x 64), 64 x 256 (4 waves of 64 x 64) and 128 x 128 (4 waves
// of 128 x 32), so mfma_tiles and mfma8_slices count its workgroups as they are.
template <bool PRELU, typename TY, bool GLU = false, bool RES = false>
static hipError_t launch_gemm8w2_t(const int8_t* x8, const uint32_t* w2, int ld8, int nblk, int K, int M, int N,
                                   const I8Epi& epi, int* slabs, int slices, hipStream_t st) {
    constexpr int kGm = 4;
    const float *scale = epi.rscale, *cscale = epi.y.cscale, *B = epi.B;
    TY* Y = static_cast<TY*>(epi.y.Y);
    const TY* R = static_cast<const TY*>(epi.R);
    const int ldy = epi.ldy;
    const float a = epi.a;
    float* sl = reinterpret_cast<float*>(slabs);
    const int bps = (nblk + slices - 1) / std::max(slices, 1);
    const int nkb = w2_kblocks(K), nt = w2_col_tiles(N);
    if (mfma_big_tiles(M, N)) {
        const int tm = (M + 127) / 128, tn = (N + 511) / 512;
        const int gm = std::min(kGm, tm);
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm8w2<8, 8, 4, PRELU, false, 1, TY, GLU, RES>), dim3(tm * tn), dim3(512), 0, st, x8, w2, ld8, M, N,
                               nblk, nkb, nt, scale, cscale, B, Y, ldy, a, tm, tn, gm, nblk, epi.G, epi.ldg, epi.act, R, epi.ldr);
        else
            hipLaunchKernelGGL((k_gemm8w2<8, 8, 4, false, true, 1>), dim3(tm * tn, slices), dim3(512), 0, st, x8, w2, ld8, M,
                               N, nblk, nkb, nt, nullptr, nullptr, nullptr, sl, N, 0.0f, tm, tn, gm, bps);
    } else if (mfma_narrow_tiles(M, N)) {
        const int tn = (N + 255) / 256;
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm8w2<4, 4, 4, PRELU, false, 2, TY, GLU, RES>), dim3(tn), dim3(256), 0, st, x8, w2, ld8, M, N, nblk,
                               nkb, nt, scale, cscale, B, Y, ldy, a, 1, tn, 1, nblk, epi.G, epi.ldg, epi.act, R, epi.ldr);
        else
            hipLaunchKernelGGL((k_gemm8w2<4, 4, 4, false, true>), dim3(tn, slices), dim3(256), 0, st, x8, w2, ld8, M, N,
                               nblk, nkb, nt, nullptr, nullptr, nullptr, sl, N, 0.0f, 1, tn, 1, bps);
    } else {
        const int tm = (M + 127) / 128, tn = (N + 127) / 128;
        const int gm = std::min(kGm, tm);
        if (slices <= 1)
            hipLaunchKernelGGL((k_gemm8w2<4, 8, 2, PRELU, false, 2, TY, GLU, RES>), dim3(tm * tn), dim3(256), 0, st, x8, w2, ld8, M, N,
                               nblk, nkb, nt, scale, cscale, B, Y, ldy, a, tm, tn, gm, nblk, epi.G, epi.ldg, epi.act, R, epi.ldr);
        else
            hipLaunchKernelGGL((k_gemm8w2<4, 8, 2, false, true>), dim3(tm * tn, slices), dim3(256), 0, st, x8, w2, ld8, M,
                               N, nblk, nkb, nt, nullptr, nullptr, nullptr, sl, N, 0.0f, tm, tn, gm, bps);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || slices <= 1) return e;
    return launch_reduce_i8(slabs, slices, M, N, epi, st);
}

// what a residual epilogue must be: no PReLU, not gated, R at a pitch of at least N, and
// an R that is Y at Y's pitch
static bool i8_res_ok(const I8Epi& e, int N) {
    return !e.prelu && !e.G && e.ldr >= N && (e.R != e.y.Y || e.ldr == e.ldy);
}

// the Y type and the PReLU of the descriptor into template arguments
template <typename F>
static hipError_t with_i8_epi(const I8Epi& e, F&& f) {
    return with_elem(e.y.ytype == kYBf16, [&](auto ty) { return with_bool(e.prelu, [&](auto pr) { return f(ty, pr); }); });
}

hipError_t mfma8_gemm(const int8_t* x8, const int8_t* w8, int ld8, int K, int M, int N, const I8Epi& e, int* slabs,
                      size_t slab_bytes, hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    const int nblk = mfma8_nblk(K);
    if (nblk < 1 || ld8 != mfma8_ldw(K) || !e.y.Y || e.G) return hipErrorInvalidValue;  // a gated call runs k_gemm8w2
    if (e.R && !i8_res_ok(e, N)) return hipErrorInvalidValue;
    const int slices = mfma8_slices(M, N, K);
    if (slices > 1 && (!slabs || slab_bytes < mfma8_slab_bytes(M, N, K))) return hipErrorInvalidValue;
    if (e.R)
        return with_elem(e.y.ytype == kYBf16, [&](auto ty) {
            return launch_gemm8_t<false, typename decltype(ty)::type, true>(x8, w8, ld8, nblk, M, N, e, slabs, slices, st);
        });
    return with_i8_epi(e, [&](auto ty, auto pr) {
        return launch_gemm8_t<decltype(pr)::value, typename decltype(ty)::type>(x8, w8, ld8, nblk, M, N, e, slabs, slices, st);
    });
}

hipError_t mfma8_gemm_w2(const int8_t* x8, const uint32_t* w2, int ld8, int K, int M, int N, const I8Epi& e, int* slabs,
                         size_t slab_bytes, hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    const int nblk = mfma8_nblk(K);
    if (nblk < 1 || ld8 != mfma8_ldw(K) || K >= kDecodeMaxK || !w2 || !e.y.Y) return hipErrorInvalidValue;
    const int slices = mfma8_slices(M, N, K);
    if (slices > 1 && (!slabs || slab_bytes < mfma8_slab_bytes(M, N, K))) return hipErrorInvalidValue;
    if (e.R) {  // a residual call: no PReLU, not gated, R at a pitch of at least N
        if (!i8_res_ok(e, N)) return hipErrorInvalidValue;
        return with_elem(e.y.ytype == kYBf16, [&](auto ty) {
            return launch_gemm8w2_t<false, typename decltype(ty)::type, false, true>(x8, w2, ld8, nblk, K, M, N, e, slabs, slices,
                                                                                    st);
        });
    }
    if (e.G) {  // the up half of a gated call: no PReLU, G at a pitch of at least N, a known activation
        if (e.prelu || e.ldg < N || (e.act != kGluRelu2 && e.act != kGluSilu)) return hipErrorInvalidValue;
        return with_elem(e.y.ytype == kYBf16, [&](auto ty) {
            return launch_gemm8w2_t<false, typename decltype(ty)::type, true>(x8, w2, ld8, nblk, K, M, N, e, slabs, slices, st);
        });
    }
    return with_i8_epi(e, [&](auto ty, auto pr) {
        return launch_gemm8w2_t<decltype(pr)::value, typename decltype(ty)::type>(x8, w2, ld8, nblk, K, M, N, e, slabs, slices,
                                                                               st);
    });
}

}  // namespace tcsc
