// tcsc_decode.hip -- the int8 decode path: tcsc_gpu_sgemm_i8
// calls of M <= 16 rows on a 2-bit image of a ternary W.
//
// At M <= 16 the product is one 16-row v_mfma_i32_16x16x64_i8 tile per 16
// columns, and the call is a stream of W.  The int8 image (k_gemm8) holds 1
// byte per weight and the merged CSC copy (k_small_m) 4 bytes per nonzero; a
// ternary weight needs 2 bits.  k_w2_from packs the int8 image into tiles of
// 16 columns x 256 k (1 KiB, the layout of tcsc_internal.h) and k_decode8
// streams them: a workgroup owns T adjacent column tiles, its 8 waves split K
// by 256-k blocks, every wave expands its 16 bytes of a tile into four int8
// fragments (one shift and one mask per dword) and issues four MFMAs per tile,
// and the partial sums meet in the LDS.
//
// The codes are c = w + 1, so the MFMAs give sum_k q c; one more MFMA per step
// against a fragment of ones gives the row sums sum_k q in the accumulator's
// own layout, and the difference is the exact S = sum_k q w as an integer.
// The epilogue is i8_out, k_gemm8's own: the same bits as the int8 MFMA path.
//
// The build-time kernels around the image live here too: k_w2_from (from the
// int8 image), k_w2_from_tcsc (packed plans, §18), and the way back in (§19):
// k_w2_check validates and counts a saved image, k_w2_unpack turns one into
// TCSC arrays.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tcsc_i8_out.h"
#include "tcsc_internal.h"
#include "tcsc_norm.h"
#include "tcsc_quant.h"
#include "tcsc_w2.h"
#include "tcsc_xsrc.h"

namespace tcsc {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Waves per workgroup (the K split) and, for A/B builds, a fixed number of
// column tiles per workgroup (0: decode_tiles_per_wg's rule).  DESIGN.md §17
// has the measurements behind 8 and the rule.
#ifndef TCSC_DEC_WAVES
#define TCSC_DEC_WAVES 8
#endif
#ifndef TCSC_DEC_TILES
#define TCSC_DEC_TILES 0
#endif
constexpr int kDecWaves = TCSC_DEC_WAVES;
constexpr int kDecTiles = TCSC_DEC_TILES;
static_assert(kDecWaves >= 1 && kDecWaves <= 16 && kDecWaves * 4 * 1024 <= 64 * 1024, "the LDS reduce of 4 tiles");
static_assert(kDecTiles == 0 || kDecTiles == 1 || kDecTiles == 2 || kDecTiles == 4, "1, 2 or 4 tiles");
// The row-tiled kernel (k_decode8r): accumulator tiles (row tiles
// x column tiles) a workgroup may hold -- 8 in registers, and kDecWaves of each
// parked in 64 KiB of LDS -- and, for A/B builds, a fixed number of column tiles
// per workgroup (0: decode_rows_tiles_per_wg's rule; capped by the first).
#ifndef TCSC_DECR_TILES
#define TCSC_DECR_TILES 0
#endif
constexpr int kDecRowsAcc = 64 / kDecWaves < 8 ? 64 / kDecWaves : 8;
constexpr int kDecRowsTiles = TCSC_DECR_TILES;
static_assert(kDecRowsAcc >= 4, "four row tiles of one column tile");
static_assert(kDecRowsTiles == 0 || kDecRowsTiles == 1 || kDecRowsTiles == 2 || kDecRowsTiles == 4, "1, 2 or 4 tiles");

// The 2-bit image from the int8 one (W8: ncols x ld8 bytes, zeros past K).  One
// thread per dword of the image, so a wave writes 1 KiB of contiguous memory;
// the reads are 16 contiguous bytes of one column (a build-time kernel).
__global__ void __launch_bounds__(256) k_w2_from(const int8_t* __restrict__ W8, int ncols, int K, int ld8, int nkb,
                                                size_t dwords, uint32_t* __restrict__ W2, int* __restrict__ bad) {
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < dwords; g += (size_t)gridDim.x * blockDim.x) {
        const size_t tile = g >> 8;  // 256 dwords per tile
        const int l = (int)(g >> 2) & 63, i = (int)g & 3;
        const int t = (int)(tile / nkb), kb = (int)(tile % nkb);
        const int col = kW2Cols * t + (l & 15), k0 = kW2Blk * kb + 64 * i + 16 * (l >> 4);
        uint32_t p = 0x55555555u;  // c = 1 everywhere: weight 0
        if (col < ncols && k0 < K) {
            const int8_t* src = W8 + (size_t)col * ld8 + k0;
            p = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int w = k0 + j < K ? (int)src[j] : 0;  // k0 + 15 < ld8: ld8 and k0 are multiples of 16
                if (w < -1 || w > 1) *bad = 1;
                p |= (uint32_t)((w + 1) & 3) << (8 * (j & 3) + 2 * (j >> 2));
            }
        }
        W2[g] = p;
    }
}

// The 2-bit image straight from the TCSC arrays (packed plans):
// no bf16 and no int8 image in between.  One workgroup per column tile and
// group of kW2BuildKb 256-k blocks: it adds the weights of its 16 columns x
// 1024 k into LDS counters (integer atomics: a +1 and a -1 at one position
// cancel, a duplicate shows as +-2, and no order of execution reaches the
// result), 16 threads per column walking that column's two index lists, then
// packs the counters in k_w2_from's bit layout.  Every workgroup of a column
// tile walks the whole columns (they need not be sorted), so the index arrays
// are read ceil(K / 1024) times, mostly from the L2; a build-time kernel.
constexpr int kW2BuildKb = 4;
constexpr int kW2BuildK = kW2BuildKb * kW2Blk;
__global__ void __launch_bounds__(256) k_w2_from_tcsc(const int* __restrict__ csp, const int* __restrict__ csn,
                                                     const int* __restrict__ rip, const int* __restrict__ rin,
                                                     int col_begin, int ncols, int K, int nkb, int nkg,
                                                     uint32_t* __restrict__ W2, int* __restrict__ bad) {
    __shared__ int w[kW2BuildK * kW2Cols];  // [k - k0][column of the tile]
    const int t = blockIdx.x / nkg, kg = blockIdx.x % nkg;
    const int k0 = kg * kW2BuildK;
    for (int i = threadIdx.x; i < kW2BuildK * kW2Cols; i += 256) w[i] = 0;
    __syncthreads();
    const int c = threadIdx.x >> 4, sub = threadIdx.x & 15, col = kW2Cols * t + c;
    if (col < ncols) {
#pragma unroll
        for (int sign = 0; sign < 2; ++sign) {
            const int* cs = sign ? csn : csp;
            const int* ri = sign ? rin : rip;
            const int e1 = cs[col_begin + col + 1];
            for (int e = cs[col_begin + col] + sub; e < e1; e += 16) {
                const int k = ri[e];
                if (k < 0 || k >= K)
                    *bad = 1;
                else if (k >= k0 && k < k0 + kW2BuildK)
                    atomicAdd(&w[(k - k0) * kW2Cols + c], sign ? -1 : 1);
            }
        }
    }
    __syncthreads();
    // thread = dword of a tile: lane l = tid >> 2, step i = tid & 3 (k_w2_from's indexing)
    const int l = threadIdx.x >> 2, i = threadIdx.x & 3;
    for (int b = 0; b < kW2BuildKb; ++b) {
        const int kb = kW2BuildKb * kg + b;
        if (kb >= nkb) break;
        const int* src = w + (kW2Blk * b + 64 * i + 16 * (l >> 4)) * kW2Cols + (l & 15);
        uint32_t p = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int v = src[j * kW2Cols];  // 0 past K and past the last column: code 1
            if (v < -1 || v > 1) *bad = 1;
            p |= (uint32_t)((v + 1) & 3) << (8 * (j & 3) + 2 * (j >> 2));
        }
        W2[((size_t)t * nkb + kb) * 256 + threadIdx.x] = p;
    }
}

// ---- reading an image back ------------------------------------
// What one dword p of an image says, given how many of its 16 positions are
// real (k < K in a column < N; the rest is padding): the +1 positions as the
// high bits of their codes, the -1 positions as the low bits, and the faults --
// a code 3 anywhere (kW2BadCode), or padding that does not hold code 1 (kW2BadPad).
struct W2Word {
    uint32_t pos, neg;  // bit 8 (j & 3) + 2 (j >> 2) + 1 for a +1 at j, + 0 for a -1
    int bad;
};
__device__ inline W2Word w2_word(uint32_t p, int nreal) {
    uint32_t m = 0;  // both bits of every real position
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < nreal) m |= 3u << (8 * (j & 3) + 2 * (j >> 2));
    W2Word r;
    r.bad = ((p & (p >> 1) & 0x55555555u) ? kW2BadCode : 0) | (((p ^ 0x55555555u) & ~m) ? kW2BadPad : 0);
    r.pos = p & 0xAAAAAAAAu & m;
    r.neg = ~(p | (p >> 1)) & 0x55555555u & m;
    return r;
}
// real positions of the dword (lane l, step i) of tile (t, kb)
__device__ inline int w2_nreal(int t, int kb, int l, int i, int ncols, int K, int* k0) {
    *k0 = kW2Blk * kb + 64 * i + 16 * (l >> 4);
    if (kW2Cols * t + (l & 15) >= ncols) return 0;
    return min(max(K - *k0, 0), 16);
}

// Validates an image and counts its weights (tcsc_gpu_plan_create_packed_image,
// tcsc_gpu_w2_to_tcsc).  One thread per dword, grid-stride, as k_w2_from; the
// +1 and -1 counts are summed per thread, then over the wave, then over the
// workgroup's four waves in the LDS, then one 64-bit integer atomicAdd per
// workgroup and sign on a grid of at most kW2CheckBlocks workgroups (the
// atomics all hit two addresses: one per wave of a thread-per-dword grid took
// longer than reading the image).  Integer adds only, so no order of execution
// shows in the counts.  counts[0] = +1, counts[1] = -1; *bad gets
// kW2BadCode and kW2BadPad OR-ed in.
constexpr unsigned kW2CheckBlocks = 1024;
__global__ void __launch_bounds__(256) k_w2_check(const uint32_t* __restrict__ W2, int ncols, int K, int nkb,
                                                 size_t dwords, unsigned long long* __restrict__ counts,
                                                 int* __restrict__ bad) {
    int np = 0, nn = 0, flags = 0;  // a full grid's wave sums are at most dwords / 256: ints hold them for any image below 2 TiB
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < dwords; g += (size_t)gridDim.x * blockDim.x) {
        const size_t tile = g >> 8;
        const int l = (int)(g >> 2) & 63, i = (int)g & 3;
        int k0;
        const W2Word w = w2_word(W2[g], w2_nreal((int)(tile / nkb), (int)(tile % nkb), l, i, ncols, K, &k0));
        np += __popc(w.pos);
        nn += __popc(w.neg);
        flags |= w.bad;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {  // every lane of the wave is here: the loop above has ended for all
        np += __shfl_xor(np, d, 64);
        nn += __shfl_xor(nn, d, 64);
        flags |= __shfl_xor(flags, d, 64);
    }
    __shared__ int part[4][3];  // the four waves' sums
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = np;
        part[threadIdx.x >> 6][1] = nn;
        part[threadIdx.x >> 6][2] = flags;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long p = 0, n = 0;
        int f = 0;
        for (int w = 0; w < 4; ++w) {
            p += (unsigned)part[w][0];
            n += (unsigned)part[w][1];
            f |= part[w][2];
        }
        if (p) atomicAdd(&counts[0], p);
        if (n) atomicAdd(&counts[1], n);
        if (f) atomicOr(bad, f);
    }
}

// The image back to TCSC (tcsc_gpu_w2_to_tcsc).  One workgroup per tile, one
// thread per dword (lane l = tid >> 2, step i = tid & 3).  Inside a 256-k block
// the ascending k order of one column is step i, then k quarter l >> 4, then j,
// so the 16 dwords of a column have ranks r = 4 i + (l >> 4).
//   FILL false: cntp / cntn[col * nkb + kb] = the +1 / -1 entries of the column
//               in this block.  An exclusive scan of these arrays (column major)
//               gives every (column, block) its absolute offset, and col_start.
//   FILL true:  each dword's entries go into an LDS copy of the block's output
//               -- its column's list, behind the entries of the dwords of lower
//               rank, in ascending j -- and the lists are then stored to offp /
//               offn[col * nkb + kb] on, 16 threads per column on consecutive
//               entries (the stores of a column are contiguous).
// Integer counters in the LDS, no atomics: every output position is determined
// by the image alone.
template <bool FILL>
__global__ void __launch_bounds__(256) k_w2_unpack(const uint32_t* __restrict__ W2, int ncols, int K, int nkb,
                                                  int* __restrict__ cntp, int* __restrict__ cntn,
                                                  const int* __restrict__ offp, const int* __restrict__ offn,
                                                  int* __restrict__ rip, int* __restrict__ rin) {
    __shared__ int sp[kW2Cols * 16], sn[kW2Cols * 16];  // [column of the tile][rank]
    __shared__ int ep[FILL ? kW2Cols * kW2Blk : 1], en[FILL ? kW2Cols * kW2Blk : 1];  // [column][entry]: k
    const int t = blockIdx.x / nkb, kb = blockIdx.x % nkb;
    const int l = threadIdx.x >> 2, i = threadIdx.x & 3, c = l & 15, r = 4 * i + (l >> 4);
    int k0;
    const int nreal = w2_nreal(t, kb, l, i, ncols, K, &k0);
    const W2Word w = w2_word(W2[(size_t)blockIdx.x * 256 + threadIdx.x], nreal);
    sp[c * 16 + r] = __popc(w.pos);
    sn[c * 16 + r] = __popc(w.neg);
    __syncthreads();
    // from here on 16 threads per column: column c2 of the tile, sub = 0 .. 15
    const int c2 = threadIdx.x >> 4, sub = threadIdx.x & 15, col2 = kW2Cols * t + c2;
    int totp = 0, totn = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        totp += sp[c2 * 16 + q];
        totn += sn[c2 * 16 + q];
    }
    const size_t o = (size_t)col2 * nkb + kb;
    if constexpr (!FILL) {
        if (sub == 0 && col2 < ncols) {
            cntp[o] = totp;
            cntn[o] = totn;
        }
    } else {
        int a = 0, b = 0;  // a column in the padding has no entries: nreal = 0 there
        for (int q = 0; q < r; ++q) {
            a += sp[c * 16 + q];
            b += sn[c * 16 + q];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int bit = 8 * (j & 3) + 2 * (j >> 2);
            if (w.pos >> (bit + 1) & 1) ep[c * kW2Blk + a++] = k0 + j;  // a, b < 256: at most 256 k a block
            if (w.neg >> bit & 1) en[c * kW2Blk + b++] = k0 + j;
        }
        __syncthreads();
        if (col2 >= ncols) return;
        int* dp = rip + offp[o];
        int* dn = rin + offn[o];
        for (int e = sub; e < totp; e += 16) dp[e] = ep[c2 * kW2Blk + e];
        for (int e = sub; e < totn; e += 16) dn[e] = en[c2 * kW2Blk + e];
    }
}

// csp / csn[j] = the offset of column j's first block, j <= ncols (the scans end in the totals)
__global__ void __launch_bounds__(256) k_w2_col_start(const int* __restrict__ offp, const int* __restrict__ offn, int ncols,
                                                     int nkb, int* __restrict__ csp, int* __restrict__ csn) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > ncols) return;
    csp[j] = offp[(size_t)j * nkb];
    csn[j] = offn[(size_t)j * nkb];
}

// k_decode8.  Grid: ceil(col tiles / T) workgroups of kDecWaves waves.  Wave w
// takes the 256-k blocks w, w + 8, ...: of each it loads the X fragments once
// (4 x 16 B per lane: row l & 15, k quarter l >> 4; rows >= M and k >= K are
// zeros and never read) and, per column tile, 16 B of image.  The next block's
// loads are issued before this block's MFMAs.  ALIGNED: X is 16-B aligned and
// K % 16 == 0, so a fragment is one 16-B load that lies wholly below K or
// wholly past it; otherwise its 16 bytes are loaded one by one, each guarded.
// K tails and column tails need nothing in the tile loop: the image's padding
// is weight 0 (code 1, cancelled by the row sums: X is zero there anyway) and
// columns >= N are computed and not stored.
//
// What k_decode8 and k_decode8q (below) share, each written once:

// The image pointers of a workgroup's T tiles: this wave's 16 bytes of tile
// (t, kb) are at wp[t] + 64 * kb (16-B units).  A workgroup's last tiles past
// the matrix read the last tile again (uniform) and are not stored.
template <int T>
__device__ __forceinline__ void decode_tile_ptrs(const uint32_t* __restrict__ W2, int t0, int ntiles, int nkb, int lane,
                                                 const u32x4* (&wp)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
        wp[t] = reinterpret_cast<const u32x4*>(W2) + (size_t)min(t0 + t, ntiles - 1) * nkb * 64 + lane;
}
template <int T>
__device__ __forceinline__ void decode_load_w(const u32x4* const (&wp)[T], int kb, u32x4 (&p)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) p[t] = __builtin_nontemporal_load(wp[t] + (size_t)kb * 64);
}

// One 256-k block: per 64-k step one MFMA against a fragment of ones (the row
// sums) and one per tile against the tile's codes (w2_codes, tcsc_w2.h).
template <int T>
__device__ __forceinline__ void decode_block(const i32x4 (&xf)[4], const u32x4 (&p)[T], i32x4 (&acc)[T], i32x4& rs) {
    const i32x4 ones = i32x4{0x01010101, 0x01010101, 0x01010101, 0x01010101};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[i], ones, rs, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[i], w2_codes(p[t][i]), acc[t], 0, 0, 0);
    }
}

// The tail.  S of this wave's K share is parked in `red` in the accumulator
// layout (register r of lane l: row 4 (l >> 4) + r, column l & 15; a wave
// without blocks adds zeros), then one thread per output -- a row's 16 T
// columns on consecutive threads -- adds the WAVES shares and stores
// i8_out(S, row_scale(row), ...).  The kernels differ in WAVES and in where
// the row scale comes from.  Every thread of the workgroup calls this.
// RES: what is stored is i8_res(value, R[row * ldr + col]), R of
// Y's type.  The thread that stores an element is the one that reads it, the
// read first, and outputs past the matrix are neither read nor stored, so
// R == Y (with ldr == ldy) reads every element once, before its store.  Y
// carries no restrict here: the kernels' own Y parameter does, except in the
// residual instantiations (I8YPtr).
template <int WAVES, int T, bool PRELU, bool RES = false, typename TY, typename RowScale>
__device__ __forceinline__ void decode_reduce_store(int* red, const i32x4 (&acc)[T], const i32x4& rs, int wave, int lane,
                                                    int t0, int M, int N, RowScale row_scale,
                                                    const float* __restrict__ cscale, const float* __restrict__ bias,
                                                    TY* Y, int ldy, float a, const TY* R = nullptr, int ldr = 0) {
    static_assert(!(RES && PRELU), "a residual call has no PReLU");
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * T + t) * 256 + r * 64 + lane] = acc[t][r] - rs[r];
    __syncthreads();
    for (int o = threadIdx.x; o < T * 256; o += WAVES * 64) {
        const int row = o / (16 * T), cg = o % (16 * T), t = cg >> 4, c = cg & 15;
        const int col = (t0 + t) * kW2Cols + c;
        if (row >= M || col >= N) continue;
        int S = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) S += red[(w * T + t) * 256 + (row & 3) * 64 + (row >> 2) * 16 + c];
        if constexpr (RES) {
            const float r = I8Y<TY>::get(R + (size_t)row * ldr + col);
            const float v = i8_out<false>(S, row_scale(row), i8_cscale(cscale, col), bias[col], 0.0f);
            I8Y<TY>::put(Y + (size_t)row * ldy + col, i8_res(v, r));
        } else {
            I8Y<TY>::put(Y + (size_t)row * ldy + col, i8_out<PRELU>(S, row_scale(row), i8_cscale(cscale, col), bias[col], a));
        }
    }
}

template <int T, bool ALIGNED, bool PRELU, typename TY, bool RES = false>
__global__ void __launch_bounds__(kDecWaves * 64) k_decode8(const int8_t* __restrict__ X,
                                                             const uint32_t* __restrict__ W2, int K, int M, int N,
                                                             int nkb, int ntiles, const float* __restrict__ scale,
                                                             const float* __restrict__ cscale,
                                                             const float* __restrict__ bias, I8YPtr<TY, RES> Y,
                                                             int ldy, float a, const TY* R = nullptr, int ldr = 0) {
    __shared__ int red[kDecWaves * T * 256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = blockIdx.x * T;
    const int xr = lane & 15, kq = lane >> 4;
    const bool row_ok = xr < M;
    const int8_t* xrow = X + (size_t)(row_ok ? xr : 0) * K;

    const u32x4* wp[T];
    decode_tile_ptrs<T>(W2, t0, ntiles, nkb, lane, wp);

    auto load = [&](int kb, i32x4 (&xf)[4], u32x4 (&p)[T]) {
        decode_load_w<T>(wp, kb, p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kW2Blk * kb + 64 * i + 16 * kq;
            xf[i] = i32x4{0, 0, 0, 0};
            if constexpr (ALIGNED) {
                if (row_ok && k < K) xf[i] = *reinterpret_cast<const i32x4*>(xrow + k);
            } else {
                if (row_ok && k < K) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const uint32_t b = k + j < K ? (uint32_t)(uint8_t)xrow[k + j] : 0u;
                        xf[i][j >> 2] |= (int)(b << (8 * (j & 3)));
                    }
                }
            }
        }
    };

    i32x4 acc[T], rs = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = i32x4{0, 0, 0, 0};

    i32x4 xf[4], xn[4];
    u32x4 p[T], pn[T];
    int kb = wave;
    if (kb < nkb) load(kb, xf, p);
    while (kb < nkb) {  // uniform
        const int nx = kb + kDecWaves;
        if (nx < nkb) load(nx, xn, pn);
        decode_block<T>(xf, p, acc, rs);
#pragma unroll
        for (int i = 0; i < 4; ++i) xf[i] = xn[i];
#pragma unroll
        for (int t = 0; t < T; ++t) p[t] = pn[t];
        kb = nx;
    }

    decode_reduce_store<kDecWaves, T, PRELU, RES>(
        red, acc, rs, wave, lane, t0, M, N, [&](int row) { return scale ? scale[row] : 1.0f; }, cscale, bias, Y, ldy, a,
        R, ldr);
}

// k_decode8q: k_quant_rows_i8 and k_decode8 in one launch, for
// fp32 (TX = float) or bf16 (TX = uint16_t) X.  k_decode8's grid, K split over 8
// waves, image loads, MFMA loop with the row-sum correction, LDS reduce and
// epilogue; what is new is where the int8 fragments come from.
//   Phase A: all 512 threads find amax[r] = max_k |x[r, k]| of the rows r < M
//   over the whole of K -- 512 / Mp threads per row (Mp = M rounded up to a power
//   of two), shuffles over the 32 lanes of a half-wave, the half-waves' maxima
//   through the LDS -- then scale and inv by quant_scales; workgroup 0 stores the
//   scales.  fmaxf is exact in any order: every workgroup gets the quantizer's bits.
//   Phase B: per 256-k block a wave quantizes the M x 256 values of its block
//   into its own 4 KiB of the LDS -- lane l takes k = 256 kb + 4 l .. + 3 of
//   every row (one 16-B or 8-B load, four quant_i8, one 4-B LDS store) -- and its
//   lanes read their 16-byte fragments from there.  A lane reads the fragment of
//   row l & 15 directly only at a cost of 64 quant_i8 per block whatever M is
//   (masked lanes issue too); through the LDS it is 4 M.  Rows >= M and k >= K
//   are never read: the first stay zero in the fragment, the second are stored
//   as zeros.  The 16-B slots of a row are swizzled by the row (slot ^ row), so
//   the 16 rows' fragment reads fall on different banks without padding.
//   The first four rows of the next block are loaded before this block's MFMAs.
// ALIGNED: XSrc<TX>::vec_ok -- 16-B loads in phase A, whole loads of a lane's
// four values in phase B; otherwise guarded scalar loads in both.
//
// NORM: the RMSNorm in front of the quantizer as well.  Phase A
// sweeps the row twice (decode_norm_sweeps): the sum of squares in tcsc_norm.h's
// order -- the 512 / Mp threads of a row are a team that owns Mp partials each
// -- then r and the maximum of |xn|; r[row] joins the scales in the LDS.  Phase
// B's store_rows applies r and gamma in front of quant_i8; a lane's four gamma
// of a block are loaded once, with the block's first rows, and serve every row.
// Everything after the fragments is the same code.  The instantiations without
// NORM read neither gamma nor eps.
constexpr int kQWaves = 8;           // the product build's K split; the staging of 16 waves would not fit 64 KiB
constexpr int kQWaveBytes = 16 * kW2Blk;  // a wave's quantized block: 16 rows x 256 k

// The two sweeps of the norm form's phase A for Mp = MP: thread tid is thread
// tid % NT of row tid / NT's team, NT = 512 / MP.  r of the thread's row and the
// thread's share of max |xn| come back (a row >= M is never read: r is of an
// empty row then and am = 0).  part: 512 floats of the LDS.  Every thread of
// the workgroup calls this.
template <typename TX, bool ALIGNED, int MP>
__device__ __forceinline__ void decode_norm_sweeps(const TX* __restrict__ X, const float* __restrict__ gamma, float eps,
                                                   int K, int M, int tid, float* part, float& r, float& am) {
    using XS = XSrc<TX>;
    constexpr int NT = kNormPartials / MP;
    const int arow = tid / NT, asub = tid % NT;
    const bool live = arow < M;
    const TX* src = X + (size_t)(live ? arow : 0) * K;
    const float node = live ? norm_ss_thread<TX, NT, ALIGNED>(src, K, asub) : 0.0f;
    r = norm_rinv(norm_ss_team<NT>(node, part, tid), K, eps);
    am = 0.0f;
    if (!live) return;
    if constexpr (ALIGNED) {  // K % 4 == 0: a piece's gamma is whole 16-B loads where gamma is aligned
        const bool gvec = (reinterpret_cast<uintptr_t>(gamma) & 15) == 0;
        for (int q = asub; q < K / XS::kVec; q += NT) {
            float f[XS::kVec];
            XS::unpack(*reinterpret_cast<const uint4*>(src + (size_t)q * XS::kVec), 1.0f, f);
            if (gvec) {
                norm_piece<XS::kVec>(f, r, gamma, q * XS::kVec);
            } else {
#pragma unroll
                for (int e = 0; e < XS::kVec; ++e) f[e] = norm_apply(f[e], r, gamma[q * XS::kVec + e]);
            }
#pragma unroll
            for (int e = 0; e < XS::kVec; ++e) am = fmaxf(am, fabsf(f[e]));
        }
    } else {
        for (int k = asub; k < K; k += NT) {
            const float x = XS::conv(src[k], 1.0f);
            am = fmaxf(am, fabsf(gamma ? norm_apply(x, r, gamma[k]) : norm_apply(x, r)));
        }
    }
}

template <typename TX, int T, bool ALIGNED, bool PRELU, typename TY, bool NORM = false, bool RES = false>
__global__ void __launch_bounds__(kQWaves * 64) k_decode8q(const TX* __restrict__ X, const uint32_t* __restrict__ W2,
                                                           int K, int M, int N, int nkb, int ntiles,
                                                           float* __restrict__ scale_out,
                                                           const float* __restrict__ cscale,
                                                           const float* __restrict__ bias, I8YPtr<TY, RES> Y,
                                                           int ldy, float a, const float* __restrict__ gamma = nullptr,
                                                           float eps = 0.0f, const TY* R = nullptr, int ldr = 0) {
    using XS = XSrc<TX>;
    constexpr int kThreads = kQWaves * 64, kHalves = kThreads / 32;
    constexpr int kRedBytes = kQWaves * T * 256 * 4, kStageBytes = kQWaves * kQWaveBytes;
    // the waves' staging blocks during the K loop, the partial sums after it (and, in the norm form's
    // phase A, the teams' 512 tree nodes)
    __shared__ __attribute__((aligned(16))) unsigned char smem[kRedBytes > kStageBytes ? kRedBytes : kStageBytes];
    __shared__ float s_part[kHalves], s_scale[kDecodeMaxM], s_inv[kDecodeMaxM];
    __shared__ float s_r[NORM ? kDecodeMaxM : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = blockIdx.x * T;

    // ---- phase A: the row maxima, scales and inverses
    {
        int sh = 0;  // Mp = 1 << sh
        while ((1 << sh) < M) ++sh;
        const int gl = 9 - sh;  // log2 of the threads per row: 512 .. 32
        static_assert(kThreads == 512 && kDecodeMaxM == 16, "512 threads over at most 16 rows: half-waves do not mix rows");
        const int arow = tid >> gl, asub = tid & ((1 << gl) - 1), G = 1 << gl;
        float am = 0.0f;
        if constexpr (NORM) {
            static_assert(kThreads == kNormPartials && kStageBytes >= kNormPartials * 4, "one thread per partial at M = 1");
            float* part = reinterpret_cast<float*>(smem);
            float r;
            switch (sh) {  // uniform
                case 0: decode_norm_sweeps<TX, ALIGNED, 1>(X, gamma, eps, K, M, tid, part, r, am); break;
                case 1: decode_norm_sweeps<TX, ALIGNED, 2>(X, gamma, eps, K, M, tid, part, r, am); break;
                case 2: decode_norm_sweeps<TX, ALIGNED, 4>(X, gamma, eps, K, M, tid, part, r, am); break;
                case 3: decode_norm_sweeps<TX, ALIGNED, 8>(X, gamma, eps, K, M, tid, part, r, am); break;
                default: decode_norm_sweeps<TX, ALIGNED, 16>(X, gamma, eps, K, M, tid, part, r, am); break;
            }
            if (arow < M && asub == 0) s_r[arow] = r;
        } else if (arow < M) {
            const TX* src = X + (size_t)arow * K;
            if constexpr (ALIGNED) {
                for (int q = asub; q < K / XS::kVec; q += G) {
                    float f[XS::kVec];
                    XS::unpack(*reinterpret_cast<const uint4*>(src + (size_t)q * XS::kVec), 1.0f, f);
#pragma unroll
                    for (int e = 0; e < XS::kVec; ++e) am = fmaxf(am, fabsf(f[e]));
                }
            } else {
                for (int k = asub; k < K; k += G) am = fmaxf(am, fabsf(XS::conv(src[k], 1.0f)));
            }
        }
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) am = fmaxf(am, __shfl_xor(am, d, 64));  // stays inside the half-wave
        if ((tid & 31) == 0) s_part[tid >> 5] = am;
        __syncthreads();
        if (tid < M) {
            const int h = G >> 5;  // half-waves per row
            float m = 0.0f;
            for (int q = 0; q < h; ++q) m = fmaxf(m, s_part[tid * h + q]);
            float sc, inv;
            quant_scales(m, sc, inv);
            s_scale[tid] = sc;
            s_inv[tid] = inv;
            if (blockIdx.x == 0) scale_out[tid] = sc;
        }
        __syncthreads();
    }

    // ---- phase B: k_decode8's loop on fragments quantized through the LDS
    const int xr = lane & 15, kq = lane >> 4;
    const bool row_ok = xr < M;
    const u32x4* wp[T];
    decode_tile_ptrs<T>(W2, t0, ntiles, nkb, lane, wp);
    unsigned char* qw = smem + wave * kQWaveBytes;

    // the lane's four values of rows j0 .. j0 + 3 of block kb, as raw bits (fp32: one per dword; bf16: two)
    constexpr int kRaw = (int)sizeof(TX);  // dwords of four values
    struct Raw {
        uint32_t w[kRaw];
    };
    auto load_rows = [&](int kb, int j0, Raw (&raw)[4]) {
        const int k = kW2Blk * kb + 4 * lane;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int d = 0; d < kRaw; ++d) raw[u].w[d] = 0;
            if (j0 + u >= M || k >= K) continue;  // the first is uniform
            const TX* src = X + (size_t)(j0 + u) * K + k;
            if constexpr (ALIGNED) {  // K % 4 == 0: the four values lie wholly below K
                if constexpr (kRaw == 4) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src);
                    raw[u].w[0] = v.x, raw[u].w[1] = v.y, raw[u].w[2] = v.z, raw[u].w[3] = v.w;
                } else {
                    const uint2 v = *reinterpret_cast<const uint2*>(src);
                    raw[u].w[0] = v.x, raw[u].w[1] = v.y;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (k + e >= K) continue;
                    if constexpr (kRaw == 4)
                        raw[u].w[e] = __float_as_uint(src[e]);
                    else
                        raw[u].w[e >> 1] |= (uint32_t)src[e] << (16 * (e & 1));
                }
            }
        }
    };
    // the norm form: gamma of the lane's four k of block kb, shared by all rows (ones past K, unused)
    [[maybe_unused]] float gm[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    [[maybe_unused]] const bool gvec = NORM && K % 4 == 0 && (reinterpret_cast<uintptr_t>(gamma) & 15) == 0;
    auto load_gamma = [&](int kb) {
        if constexpr (NORM) {
            const int k = kW2Blk * kb + 4 * lane;
            if (!gamma) return;  // uniform
            if (gvec) {          // uniform; the four lie wholly below K or wholly past it
                if (k < K) {
                    const float4 g = *reinterpret_cast<const float4*>(gamma + k);
                    gm[0] = g.x, gm[1] = g.y, gm[2] = g.z, gm[3] = g.w;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < K) gm[e] = gamma[k + e];
            }
        }
    };
    // quantized and stored: byte e of the dword is value k + e, zero at k + e >= K
    auto store_rows = [&](int kb, int j0, const Raw (&raw)[4]) {
        const int k = kW2Blk * kb + 4 * lane;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = j0 + u;
            if (row >= M) break;  // uniform
            const float inv = s_inv[row];
            [[maybe_unused]] const float r = NORM ? s_r[row] : 1.0f;
            uint32_t o = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x;
                if constexpr (kRaw == 4)
                    x = __uint_as_float(raw[u].w[e]);
                else
                    x = XS::conv((TX)(raw[u].w[e >> 1] >> (16 * (e & 1))), 1.0f);
                if constexpr (NORM) x = gamma ? norm_apply(x, r, gm[e]) : norm_apply(x, r);
                const uint32_t q = (uint32_t)quant_i8(x, inv) & 0xffu;
                if (ALIGNED ? k < K : k + e < K) o |= q << (8 * e);
            }
            *reinterpret_cast<uint32_t*>(qw + row * kW2Blk + (((lane >> 2) ^ row) << 4) + 4 * (lane & 3)) = o;
        }
    };
    auto stage_rest = [&](int kb, Raw (&raw)[4]) {  // rows 4 .. M - 1, four at a time
        for (int j0 = 4; j0 < M; j0 += 4) {
            load_rows(kb, j0, raw);
            store_rows(kb, j0, raw);
        }
    };
    // the wave's own stores, read by its other lanes: LDS operations of one wave execute in order
    auto fragments = [&](i32x4 (&xf)[4]) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xf[i] = i32x4{0, 0, 0, 0};
            if (row_ok) xf[i] = *reinterpret_cast<const i32x4*>(qw + xr * kW2Blk + (((4 * i + kq) ^ xr) << 4));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    i32x4 acc[T], rs = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = i32x4{0, 0, 0, 0};

    i32x4 xf[4];
    u32x4 p[T], pn[T];
    Raw raw[4];
    int kb = wave;
    if (kb < nkb) {
        decode_load_w<T>(wp, kb, p);
        load_gamma(kb);
        load_rows(kb, 0, raw);
        store_rows(kb, 0, raw);
        stage_rest(kb, raw);
        fragments(xf);
    }
    while (kb < nkb) {  // uniform
        const int nx = kb + kQWaves;
        if (nx < nkb) {
            decode_load_w<T>(wp, nx, pn);
            load_gamma(nx);  // this block's staging is done: its gamma is free
            load_rows(nx, 0, raw);
        }
        decode_block<T>(xf, p, acc, rs);
        if (nx < nkb) {  // this block's fragments are in registers: its staging block is free
            store_rows(nx, 0, raw);
            stage_rest(nx, raw);
            fragments(xf);
#pragma unroll
            for (int t = 0; t < T; ++t) p[t] = pn[t];
        }
        kb = nx;
    }

    __syncthreads();  // every wave is done with its staging block: the partial sums take the memory
    decode_reduce_store<kQWaves, T, PRELU, RES>(
        reinterpret_cast<int*>(smem), acc, rs, wave, lane, t0, M, N, [&](int row) { return s_scale[row]; }, cscale, bias, Y,
        ldy, a, R, ldr);
}

// ---- the gated forms: act(X Wg) (X Wu) in one launch ---------------
// k_decode8g and k_decode8qg are k_decode8 and k_decode8q on two images of one
// K x N shape: a workgroup owns TG column tiles and streams the 2 TG tiles of the
// gate and the up image against one set of X fragments and one row-sum MFMA per
// step (decode_load_w / decode_block at T = 2 TG), and the tail multiplies the
// two values.  k_decode8 and k_decode8q above are left as they are, text and
// code: their bodies up to the tail are repeated below (decode8g_sums,
// decode8qg_body) because the same text behind a function boundary moved the
// register allocation of the existing instantiations (a few VGPRs, and 36 B of
// scratch back into the T = 4 norm form), which §24 rules out.
//
// The gated tail: `red` holds the shares of a workgroup's TG gate
// tiles (t < TG) and then of its TG up tiles, and one thread per output adds the
// WAVES shares of Sg and of Su, applies i8_out to each and i8_glu to the pair, and
// does the one store.  Every thread of the workgroup calls this.
struct GluEpi {
    const float *cg, *bg, *cu, *bu;  // the column scales (null: ones) and biases of the gate and up halves
    int act;
};
template <int WAVES, int TG, typename TY, typename RowScale>
__device__ __forceinline__ void decode_reduce_store_glu(int* red, const i32x4 (&acc)[2 * TG], const i32x4& rs, int wave,
                                                        int lane, int t0, int M, int N, RowScale row_scale,
                                                        const GluEpi& e, TY* __restrict__ Y, int ldy) {
    constexpr int T = 2 * TG;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * T + t) * 256 + r * 64 + lane] = acc[t][r] - rs[r];
    __syncthreads();
    for (int o = threadIdx.x; o < TG * 256; o += WAVES * 64) {
        const int row = o / (16 * TG), cg = o % (16 * TG), t = cg >> 4, c = cg & 15;
        const int col = (t0 + t) * kW2Cols + c;
        if (row >= M || col >= N) continue;
        int Sg = 0, Su = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            Sg += red[(w * T + t) * 256 + (row & 3) * 64 + (row >> 2) * 16 + c];
            Su += red[(w * T + TG + t) * 256 + (row & 3) * 64 + (row >> 2) * 16 + c];
        }
        const float s = row_scale(row);
        const float g = i8_out<false>(Sg, s, i8_cscale(e.cg, col), e.bg[col], 0.0f);
        const float u = i8_out<false>(Su, s, i8_cscale(e.cu, col), e.bu[col], 0.0f);
        I8Y<TY>::put(Y + (size_t)row * ldy + col, i8_glu(g, u, e.act));
    }
}

// The two images of a gated launch: a workgroup's tiles are TG adjacent ones of
// the gate image (wp[0 .. TG)) and the same TG of the up image (wp[TG .. 2 TG)),
// decode_tile_ptrs once per image.  t0 is the workgroup's first column tile.
template <int TG>
struct DecodeImg2 {
    static constexpr int T = 2 * TG, kColTiles = TG;
    const uint32_t *Wg, *Wu;
    __device__ __forceinline__ void ptrs(int t0, int ntiles, int nkb, int lane, const u32x4* (&wp)[T]) const {
        const u32x4 *g[TG], *u[TG];
        decode_tile_ptrs<TG>(Wg, t0, ntiles, nkb, lane, g);
        decode_tile_ptrs<TG>(Wu, t0, ntiles, nkb, lane, u);
#pragma unroll
        for (int t = 0; t < TG; ++t) wp[t] = g[t], wp[TG + t] = u[t];
    }
};

// k_decode8's body up to the tail: this wave's share of sum q c of the workgroup's
// IMG::T tiles in acc and of the row sums in rs.
template <bool ALIGNED, typename IMG>
__device__ __forceinline__ void decode8g_sums(const int8_t* __restrict__ X, const IMG& img, int K, int M, int nkb,
                                             int ntiles, int t0, int wave, int lane, i32x4 (&acc)[IMG::T], i32x4& rs) {
    constexpr int T = IMG::T;
    const int xr = lane & 15, kq = lane >> 4;
    const bool row_ok = xr < M;
    const int8_t* xrow = X + (size_t)(row_ok ? xr : 0) * K;

    const u32x4* wp[T];
    img.ptrs(t0, ntiles, nkb, lane, wp);

    auto load = [&](int kb, i32x4 (&xf)[4], u32x4 (&p)[T]) {
        decode_load_w<T>(wp, kb, p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kW2Blk * kb + 64 * i + 16 * kq;
            xf[i] = i32x4{0, 0, 0, 0};
            if constexpr (ALIGNED) {
                if (row_ok && k < K) xf[i] = *reinterpret_cast<const i32x4*>(xrow + k);
            } else {
                if (row_ok && k < K) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const uint32_t b = k + j < K ? (uint32_t)(uint8_t)xrow[k + j] : 0u;
                        xf[i][j >> 2] |= (int)(b << (8 * (j & 3)));
                    }
                }
            }
        }
    };

    rs = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = i32x4{0, 0, 0, 0};

    i32x4 xf[4], xn[4];
    u32x4 p[T], pn[T];
    int kb = wave;
    if (kb < nkb) load(kb, xf, p);
    while (kb < nkb) {  // uniform
        const int nx = kb + kDecWaves;
        if (nx < nkb) load(nx, xn, pn);
        decode_block<T>(xf, p, acc, rs);
#pragma unroll
        for (int i = 0; i < 4; ++i) xf[i] = xn[i];
#pragma unroll
        for (int t = 0; t < T; ++t) p[t] = pn[t];
        kb = nx;
    }
}

// The gated k_decode8; act is a uniform branch in the tail.
template <int TG, bool ALIGNED, typename TY>
__global__ void __launch_bounds__(kDecWaves * 64) k_decode8g(const int8_t* __restrict__ X,
                                                              const uint32_t* __restrict__ Wg,
                                                              const uint32_t* __restrict__ Wu, int K, int M, int N,
                                                              int nkb, int ntiles, const float* __restrict__ scale,
                                                              GluEpi e, TY* __restrict__ Y, int ldy) {
    __shared__ int red[kDecWaves * 2 * TG * 256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = blockIdx.x * TG;
    i32x4 acc[2 * TG], rs;
    decode8g_sums<ALIGNED>(X, DecodeImg2<TG>{Wg, Wu}, K, M, nkb, ntiles, t0, wave, lane, acc, rs);
    decode_reduce_store_glu<kDecWaves, TG>(
        red, acc, rs, wave, lane, t0, M, N, [&](int row) { return scale ? scale[row] : 1.0f; }, e, Y, ldy);
}

// k_decode8q's body up to the tail -- phase A and the whole of phase B, the norm
// form included, run once for both matrices: tail(red, s_scale, acc, rs, wave,
// lane, t0) gets the LDS the partial sums take, the rows' scales in the LDS and
// this wave's sums.
template <typename TX, bool ALIGNED, bool NORM, typename IMG, typename Tail>
__device__ __forceinline__ void decode8qg_body(const TX* __restrict__ X, const IMG& img, int K, int M, int nkb,
                                              int ntiles, float* __restrict__ scale_out,
                                              const float* __restrict__ gamma, float eps, Tail tail) {
    using XS = XSrc<TX>;
    constexpr int T = IMG::T;
    constexpr int kThreads = kQWaves * 64, kHalves = kThreads / 32;
    constexpr int kRedBytes = kQWaves * T * 256 * 4, kStageBytes = kQWaves * kQWaveBytes;
    // the waves' staging blocks during the K loop, the partial sums after it (and, in the norm form's
    // phase A, the teams' 512 tree nodes)
    __shared__ __attribute__((aligned(16))) unsigned char smem[kRedBytes > kStageBytes ? kRedBytes : kStageBytes];
    __shared__ float s_part[kHalves], s_scale[kDecodeMaxM], s_inv[kDecodeMaxM];
    __shared__ float s_r[NORM ? kDecodeMaxM : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = blockIdx.x * IMG::kColTiles;

    // ---- phase A: the row maxima, scales and inverses
    {
        int sh = 0;  // Mp = 1 << sh
        while ((1 << sh) < M) ++sh;
        const int gl = 9 - sh;  // log2 of the threads per row: 512 .. 32
        static_assert(kThreads == 512 && kDecodeMaxM == 16, "512 threads over at most 16 rows: half-waves do not mix rows");
        const int arow = tid >> gl, asub = tid & ((1 << gl) - 1), G = 1 << gl;
        float am = 0.0f;
        if constexpr (NORM) {
            static_assert(kThreads == kNormPartials && kStageBytes >= kNormPartials * 4, "one thread per partial at M = 1");
            float* part = reinterpret_cast<float*>(smem);
            float r;
            switch (sh) {  // uniform
                case 0: decode_norm_sweeps<TX, ALIGNED, 1>(X, gamma, eps, K, M, tid, part, r, am); break;
                case 1: decode_norm_sweeps<TX, ALIGNED, 2>(X, gamma, eps, K, M, tid, part, r, am); break;
                case 2: decode_norm_sweeps<TX, ALIGNED, 4>(X, gamma, eps, K, M, tid, part, r, am); break;
                case 3: decode_norm_sweeps<TX, ALIGNED, 8>(X, gamma, eps, K, M, tid, part, r, am); break;
                default: decode_norm_sweeps<TX, ALIGNED, 16>(X, gamma, eps, K, M, tid, part, r, am); break;
            }
            if (arow < M && asub == 0) s_r[arow] = r;
        } else if (arow < M) {
            const TX* src = X + (size_t)arow * K;
            if constexpr (ALIGNED) {
                for (int q = asub; q < K / XS::kVec; q += G) {
                    float f[XS::kVec];
                    XS::unpack(*reinterpret_cast<const uint4*>(src + (size_t)q * XS::kVec), 1.0f, f);
#pragma unroll
                    for (int e = 0; e < XS::kVec; ++e) am = fmaxf(am, fabsf(f[e]));
                }
            } else {
                for (int k = asub; k < K; k += G) am = fmaxf(am, fabsf(XS::conv(src[k], 1.0f)));
            }
        }
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) am = fmaxf(am, __shfl_xor(am, d, 64));  // stays inside the half-wave
        if ((tid & 31) == 0) s_part[tid >> 5] = am;
        __syncthreads();
        if (tid < M) {
            const int h = G >> 5;  // half-waves per row
            float m = 0.0f;
            for (int q = 0; q < h; ++q) m = fmaxf(m, s_part[tid * h + q]);
            float sc, inv;
            quant_scales(m, sc, inv);
            s_scale[tid] = sc;
            s_inv[tid] = inv;
            if (blockIdx.x == 0) scale_out[tid] = sc;
        }
        __syncthreads();
    }

    // ---- phase B: k_decode8's loop on fragments quantized through the LDS
    const int xr = lane & 15, kq = lane >> 4;
    const bool row_ok = xr < M;
    const u32x4* wp[T];
    img.ptrs(t0, ntiles, nkb, lane, wp);
    unsigned char* qw = smem + wave * kQWaveBytes;

    // the lane's four values of rows j0 .. j0 + 3 of block kb, as raw bits (fp32: one per dword; bf16: two)
    constexpr int kRaw = (int)sizeof(TX);  // dwords of four values
    struct Raw {
        uint32_t w[kRaw];
    };
    auto load_rows = [&](int kb, int j0, Raw (&raw)[4]) {
        const int k = kW2Blk * kb + 4 * lane;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int d = 0; d < kRaw; ++d) raw[u].w[d] = 0;
            if (j0 + u >= M || k >= K) continue;  // the first is uniform
            const TX* src = X + (size_t)(j0 + u) * K + k;
            if constexpr (ALIGNED) {  // K % 4 == 0: the four values lie wholly below K
                if constexpr (kRaw == 4) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src);
                    raw[u].w[0] = v.x, raw[u].w[1] = v.y, raw[u].w[2] = v.z, raw[u].w[3] = v.w;
                } else {
                    const uint2 v = *reinterpret_cast<const uint2*>(src);
                    raw[u].w[0] = v.x, raw[u].w[1] = v.y;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (k + e >= K) continue;
                    if constexpr (kRaw == 4)
                        raw[u].w[e] = __float_as_uint(src[e]);
                    else
                        raw[u].w[e >> 1] |= (uint32_t)src[e] << (16 * (e & 1));
                }
            }
        }
    };
    // the norm form: gamma of the lane's four k of block kb, shared by all rows (ones past K, unused)
    [[maybe_unused]] float gm[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    [[maybe_unused]] const bool gvec = NORM && K % 4 == 0 && (reinterpret_cast<uintptr_t>(gamma) & 15) == 0;
    auto load_gamma = [&](int kb) {
        if constexpr (NORM) {
            const int k = kW2Blk * kb + 4 * lane;
            if (!gamma) return;  // uniform
            if (gvec) {          // uniform; the four lie wholly below K or wholly past it
                if (k < K) {
                    const float4 g = *reinterpret_cast<const float4*>(gamma + k);
                    gm[0] = g.x, gm[1] = g.y, gm[2] = g.z, gm[3] = g.w;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < K) gm[e] = gamma[k + e];
            }
        }
    };
    // quantized and stored: byte e of the dword is value k + e, zero at k + e >= K
    auto store_rows = [&](int kb, int j0, const Raw (&raw)[4]) {
        const int k = kW2Blk * kb + 4 * lane;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = j0 + u;
            if (row >= M) break;  // uniform
            const float inv = s_inv[row];
            [[maybe_unused]] const float r = NORM ? s_r[row] : 1.0f;
            uint32_t o = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x;
                if constexpr (kRaw == 4)
                    x = __uint_as_float(raw[u].w[e]);
                else
                    x = XS::conv((TX)(raw[u].w[e >> 1] >> (16 * (e & 1))), 1.0f);
                if constexpr (NORM) x = gamma ? norm_apply(x, r, gm[e]) : norm_apply(x, r);
                const uint32_t q = (uint32_t)quant_i8(x, inv) & 0xffu;
                if (ALIGNED ? k < K : k + e < K) o |= q << (8 * e);
            }
            *reinterpret_cast<uint32_t*>(qw + row * kW2Blk + (((lane >> 2) ^ row) << 4) + 4 * (lane & 3)) = o;
        }
    };
    auto stage_rest = [&](int kb, Raw (&raw)[4]) {  // rows 4 .. M - 1, four at a time
        for (int j0 = 4; j0 < M; j0 += 4) {
            load_rows(kb, j0, raw);
            store_rows(kb, j0, raw);
        }
    };
    // the wave's own stores, read by its other lanes: LDS operations of one wave execute in order
    auto fragments = [&](i32x4 (&xf)[4]) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xf[i] = i32x4{0, 0, 0, 0};
            if (row_ok) xf[i] = *reinterpret_cast<const i32x4*>(qw + xr * kW2Blk + (((4 * i + kq) ^ xr) << 4));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    i32x4 acc[T], rs = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = i32x4{0, 0, 0, 0};

    i32x4 xf[4];
    u32x4 p[T], pn[T];
    Raw raw[4];
    int kb = wave;
    if (kb < nkb) {
        decode_load_w<T>(wp, kb, p);
        load_gamma(kb);
        load_rows(kb, 0, raw);
        store_rows(kb, 0, raw);
        stage_rest(kb, raw);
        fragments(xf);
    }
    while (kb < nkb) {  // uniform
        const int nx = kb + kQWaves;
        if (nx < nkb) {
            decode_load_w<T>(wp, nx, pn);
            load_gamma(nx);  // this block's staging is done: its gamma is free
            load_rows(nx, 0, raw);
        }
        decode_block<T>(xf, p, acc, rs);
        if (nx < nkb) {  // this block's fragments are in registers: its staging block is free
            store_rows(nx, 0, raw);
            stage_rest(nx, raw);
            fragments(xf);
#pragma unroll
            for (int t = 0; t < T; ++t) p[t] = pn[t];
        }
        kb = nx;
    }

    __syncthreads();  // every wave is done with its staging block: the partial sums take the memory
    tail(reinterpret_cast<int*>(smem), s_scale, acc, rs, wave, lane, t0);
}

// The gated k_decode8q.
template <typename TX, int TG, bool ALIGNED, typename TY, bool NORM>
__global__ void __launch_bounds__(kQWaves * 64) k_decode8qg(const TX* __restrict__ X, const uint32_t* __restrict__ Wg,
                                                            const uint32_t* __restrict__ Wu, int K, int M, int N,
                                                            int nkb, int ntiles, float* __restrict__ scale_out,
                                                            GluEpi e, TY* __restrict__ Y, int ldy,
                                                            const float* __restrict__ gamma, float eps) {
    decode8qg_body<TX, ALIGNED, NORM>(
        X, DecodeImg2<TG>{Wg, Wu}, K, M, nkb, ntiles, scale_out, gamma, eps,
        [&](int* red, const float* s_scale, const i32x4(&acc)[2 * TG], const i32x4& rs, int wave, int lane, int t0) {
            decode_reduce_store_glu<kQWaves, TG>(
                red, acc, rs, wave, lane, t0, M, N, [&](int row) { return s_scale[row]; }, e, Y, ldy);
        });
}

// ---- the grouped forms: up to four matrices on one X in one launch ----
// k_decode8m and k_decode8qm are k_decode8 and k_decode8q (without PReLU and
// without the norm) on a grid that is the concatenation of the members'
// workgroups: member i owns ceil(tiles_i / T) consecutive blocks from
// m[i].first on, and all T tiles of a block lie in one member (its last block
// reads its last tile again: decode_tile_ptrs).  The members differ in image,
// column count, column scales, bias, Y and pitch; K, M, X, the row scales and
// the Y type are the launch's.  The table is a kernel argument by value and a
// block finds its member by comparing blockIdx.x with the first blocks of
// members 1 .. 3 (INT_MAX for a slot past the group's count): compares and
// selects over the four slots, so every field stays in scalar registers -- an
// array indexed by a run-time member number would be copied to scratch.
// From there the bodies are decode8g_sums / decode8qg_body on one image and
// decode_reduce_store as the tail.
struct GroupSlot {
    const uint32_t* W2;
    const float *cscale, *bias;
    void* Y;
    int N, ntiles, ldy, first;
};
struct GroupTable {
    GroupSlot m[kGroupMax];
};
static_assert(kGroupMax == 4, "decode_group_slot selects over four slots");
__device__ __forceinline__ GroupSlot decode_group_slot(const GroupTable& g, int block) {
    const bool a1 = block >= g.m[1].first, a2 = block >= g.m[2].first, a3 = block >= g.m[3].first;  // uniform
    // The empty asm pins each chosen value in scalar registers here: without it the selects sink to the
    // tail and all four slots stay live across the K loop (SGPR spills in k_decode8qm).
    auto pick = [&](auto s0, auto s1, auto s2, auto s3) {
        auto v = a3 ? s3 : a2 ? s2 : a1 ? s1 : s0;
        asm volatile("" : "+s"(v));
        return v;
    };
    GroupSlot s;
    s.W2 = pick(g.m[0].W2, g.m[1].W2, g.m[2].W2, g.m[3].W2);
    s.cscale = pick(g.m[0].cscale, g.m[1].cscale, g.m[2].cscale, g.m[3].cscale);
    s.bias = pick(g.m[0].bias, g.m[1].bias, g.m[2].bias, g.m[3].bias);
    s.Y = pick(g.m[0].Y, g.m[1].Y, g.m[2].Y, g.m[3].Y);
    s.N = pick(g.m[0].N, g.m[1].N, g.m[2].N, g.m[3].N);
    s.ntiles = pick(g.m[0].ntiles, g.m[1].ntiles, g.m[2].ntiles, g.m[3].ntiles);
    s.ldy = pick(g.m[0].ldy, g.m[1].ldy, g.m[2].ldy, g.m[3].ldy);
    s.first = pick(0, g.m[1].first, g.m[2].first, g.m[3].first);
    return s;
}

// The one image of a grouped workgroup: TT adjacent tiles of the member's image.
// tbase is the tile number the body gives the member's first tile (blockIdx.x
// * TT there): ptrs takes it off again.
template <int TT>
struct DecodeImg1 {
    static constexpr int T = TT, kColTiles = TT;
    const uint32_t* W;
    int tbase;
    __device__ __forceinline__ void ptrs(int t0, int ntiles, int nkb, int lane, const u32x4* (&wp)[T]) const {
        decode_tile_ptrs<TT>(W, t0 - tbase, ntiles, nkb, lane, wp);
    }
};

// The grouped k_decode8.
template <int T, bool ALIGNED, typename TY>
__global__ void __launch_bounds__(kDecWaves * 64) k_decode8m(const int8_t* __restrict__ X, GroupTable g, int K, int M,
                                                              int nkb, const float* __restrict__ scale) {
    __shared__ int red[kDecWaves * T * 256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const GroupSlot s = decode_group_slot(g, blockIdx.x);
    const int t0 = (blockIdx.x - s.first) * T;  // in the member's own tiles
    i32x4 acc[T], rs;
    decode8g_sums<ALIGNED>(X, DecodeImg1<T>{s.W2, 0}, K, M, nkb, s.ntiles, t0, wave, lane, acc, rs);
    decode_reduce_store<kDecWaves, T, false>(
        red, acc, rs, wave, lane, t0, M, s.N, [&](int row) { return scale ? scale[row] : 1.0f; }, s.cscale, s.bias,
        static_cast<TY*>(s.Y), s.ldy, 0.0f);
}

// The grouped k_decode8q: phase A and phase B are k_decode8q's, and the launch's
// block 0 stores the row scales once.  No norm form.
template <typename TX, int T, bool ALIGNED, typename TY>
__global__ void __launch_bounds__(kQWaves * 64) k_decode8qm(const TX* __restrict__ X, GroupTable g, int K, int M,
                                                            int nkb, float* __restrict__ scale_out) {
    const GroupSlot s = decode_group_slot(g, blockIdx.x);
    const int tbase = s.first * T;
    decode8qg_body<TX, ALIGNED, false>(
        X, DecodeImg1<T>{s.W2, tbase}, K, M, nkb, s.ntiles, scale_out, nullptr, 0.0f,
        [&](int* red, const float* s_scale, const i32x4(&acc)[T], const i32x4& rs, int wave, int lane, int t0) {
            decode_reduce_store<kQWaves, T, false>(
                red, acc, rs, wave, lane, t0 - tbase, M, s.N, [&](int row) { return s_scale[row]; }, s.cscale, s.bias,
                static_cast<TY*>(s.Y), s.ldy, 0.0f);
        });
}

// ---- the row-tiled form: 17 .. 64 rows in one pass over the image ----
// k_decode8r is k_decode8 with RT 16-row tiles per workgroup: the grid, the K
// split over the waves, the image loads and w2_codes are k_decode8's, and every
// expanded fragment of the image feeds RT MFMAs instead of one.  Per 256-k block
// a wave loads RT x 4 X fragments -- lane l reads rows 16 rt + (l & 15), rows
// >= M and k >= K are zeros and never read -- and its T image pieces; the row
// sums take one MFMA per step and row tile (rs[RT]), the codes one per step,
// row tile and column tile (acc[RT][T]).  A row tile without a row below M
// issues no MFMA (a uniform branch: M is the launch's).
// The prefetch: X travels in batches of H steps with two sets of registers, one
// in use and one in flight.  At RT = 2 a batch is the block (H = 4): the next
// block's X and image are issued before this block's MFMAs, k_decode8's
// pipeline, the two sets swapping roles from block to block (the loop is
// unrolled by two instead of copying 32 registers).  At RT = 4 two sets of a
// whole block are 128 registers and the kernel spilled (the 512 threads leave
// 256 a wave), so a batch is half a block (H = 2): the second half's fragments
// are in flight during the first half's MFMAs and the next block's first half
// during the second's; the image stays one block ahead.
// RT T <= 8 (kDecRowsAcc): the partial sums of all row tiles are parked at once in 8 RT T KiB
// of the LDS, 64 KiB at the most, so the tail has k_decode8's one barrier.
// k_decode8 and its siblings above are left as they are, text and code.
template <int RT, int T, int H, int B>  // steps H B .. H B + H - 1 of a block: batch B of its X
__device__ __forceinline__ void decode_steps_rows(const i32x4 (&xf)[RT][H], const u32x4 (&p)[T], int M,
                                                  i32x4 (&acc)[RT][T], i32x4 (&rs)[RT]) {
    const i32x4 ones = i32x4{0x01010101, 0x01010101, 0x01010101, 0x01010101};
#pragma unroll
    for (int ii = 0; ii < H; ++ii) {
        i32x4 c[T];
#pragma unroll
        for (int t = 0; t < T; ++t) c[t] = w2_codes(p[t][H * B + ii]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            if (16 * rt >= M) continue;  // uniform
            rs[rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[rt][ii], ones, rs[rt], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < T; ++t) acc[rt][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[rt][ii], c[t], acc[rt][t], 0, 0, 0);
        }
    }
}

// decode_reduce_store over RT row tiles: row r of tile rt is row 16 rt + r of Y
// and of R.  `red` holds WAVES x RT x T accumulator tiles; one thread per
// output -- a row's 16 T columns on consecutive threads -- adds the WAVES
// shares, reads R first where there is one, and stores.
template <int WAVES, int RT, int T, bool PRELU, bool RES, typename TY>
__device__ __forceinline__ void decode_reduce_store_rows(int* red, const i32x4 (&acc)[RT][T], const i32x4 (&rs)[RT],
                                                         int wave, int lane, int t0, int M, int N,
                                                         const float* __restrict__ scale,
                                                         const float* __restrict__ cscale,
                                                         const float* __restrict__ bias, TY* Y, int ldy, float a,
                                                         const TY* R, int ldr) {
    static_assert(!(RES && PRELU), "a residual call has no PReLU");
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[((wave * RT + rt) * T + t) * 256 + r * 64 + lane] = acc[rt][t][r] - rs[rt][r];
    __syncthreads();
    for (int o = threadIdx.x; o < RT * T * 256; o += WAVES * 64) {
        const int row = o / (16 * T), cg = o % (16 * T), t = cg >> 4, c = cg & 15;
        const int col = (t0 + t) * kW2Cols + c;
        if (row >= M || col >= N) continue;
        const int rt = row >> 4, r = row & 15;
        int S = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) S += red[((w * RT + rt) * T + t) * 256 + (r & 3) * 64 + (r >> 2) * 16 + c];
        const float rsc = scale ? scale[row] : 1.0f;
        if constexpr (RES) {
            const float res = I8Y<TY>::get(R + (size_t)row * ldr + col);
            const float v = i8_out<false>(S, rsc, i8_cscale(cscale, col), bias[col], 0.0f);
            I8Y<TY>::put(Y + (size_t)row * ldy + col, i8_res(v, res));
        } else {
            I8Y<TY>::put(Y + (size_t)row * ldy + col, i8_out<PRELU>(S, rsc, i8_cscale(cscale, col), bias[col], a));
        }
    }
}

template <int RT, int T, bool ALIGNED, bool PRELU, typename TY, bool RES = false>
__global__ void __launch_bounds__(kDecWaves * 64) k_decode8r(const int8_t* __restrict__ X,
                                                              const uint32_t* __restrict__ W2, int K, int M, int N,
                                                              int nkb, int ntiles, const float* __restrict__ scale,
                                                              const float* __restrict__ cscale,
                                                              const float* __restrict__ bias, I8YPtr<TY, RES> Y,
                                                              int ldy, float a, const TY* R = nullptr, int ldr = 0) {
    static_assert(RT >= 2 && RT * T <= kDecRowsAcc, "all row tiles' sums at once in 64 KiB");
    __shared__ int red[kDecWaves * RT * T * 256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = blockIdx.x * T;
    const int xr = lane & 15, kq = lane >> 4;
    bool row_ok[RT];
    const int8_t* xrow[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        row_ok[rt] = 16 * rt + xr < M;
        xrow[rt] = X + (size_t)(row_ok[rt] ? 16 * rt + xr : 0) * K;
    }

    const u32x4* wp[T];
    decode_tile_ptrs<T>(W2, t0, ntiles, nkb, lane, wp);

    constexpr int H = RT > 2 ? 2 : 4;  // steps of an X batch
    auto load_x = [&](int kb, int batch, i32x4 (&xf)[RT][H]) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int ii = 0; ii < H; ++ii) {
                const int k = kW2Blk * kb + 64 * (H * batch + ii) + 16 * kq;
                xf[rt][ii] = i32x4{0, 0, 0, 0};
                if constexpr (ALIGNED) {
                    if (row_ok[rt] && k < K) xf[rt][ii] = *reinterpret_cast<const i32x4*>(xrow[rt] + k);
                } else {
                    if (row_ok[rt] && k < K) {
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const uint32_t b = k + j < K ? (uint32_t)(uint8_t)xrow[rt][k + j] : 0u;
                            xf[rt][ii][j >> 2] |= (int)(b << (8 * (j & 3)));
                        }
                    }
                }
            }
        }
    };

    i32x4 acc[RT][T], rs[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        rs[rt] = i32x4{0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < T; ++t) acc[rt][t] = i32x4{0, 0, 0, 0};
    }

    i32x4 xa[RT][H], xb[RT][H];
    u32x4 pa[T], pb[T];
    int kb = wave;
    if (kb < nkb) {
        decode_load_w<T>(wp, kb, pa);
        load_x(kb, 0, xa);
    }
    while (kb < nkb) {  // uniform
        int nx = kb + kDecWaves;
        if constexpr (H == 4) {  // two blocks a round: a's, then b's
            if (nx < nkb) {
                decode_load_w<T>(wp, nx, pb);
                load_x(nx, 0, xb);
            }
            decode_steps_rows<RT, T, 4, 0>(xa, pa, M, acc, rs);
            kb = nx;
            if (kb >= nkb) break;
            nx = kb + kDecWaves;
            if (nx < nkb) {
                decode_load_w<T>(wp, nx, pa);
                load_x(nx, 0, xa);
            }
            decode_steps_rows<RT, T, 4, 0>(xb, pb, M, acc, rs);
        } else {  // one block a round: its first half in a, its second in b
            load_x(kb, 1, xb);
            if (nx < nkb) decode_load_w<T>(wp, nx, pb);
            decode_steps_rows<RT, T, 2, 0>(xa, pa, M, acc, rs);
            if (nx < nkb) load_x(nx, 0, xa);
            decode_steps_rows<RT, T, 2, 1>(xb, pa, M, acc, rs);
#pragma unroll
            for (int t = 0; t < T; ++t) pa[t] = pb[t];
        }
        kb = nx;
    }

    decode_reduce_store_rows<kDecWaves, RT, T, PRELU, RES, TY>(red, acc, rs, wave, lane, t0, M, N, scale, cscale, bias, Y,
                                                               ldy, a, R, ldr);
}

// ---- the gated and grouped row-tiled forms -------------------------
// k_decode8gr and k_decode8mr are k_decode8g and k_decode8m with RT 16-row tiles
// per workgroup, on an int8 X alone: the images, the grids, the member table and
// the epilogues are theirs, the K loop and its prefetch are k_decode8r's.
// k_decode8r above is left as it is, text and code (§24's finding: the same text
// behind a function boundary moves the register allocation of the existing
// instantiations), so its body up to the tail is repeated here once, over an
// image type, for both new kernels: decode8r_body is decode8g_sums over xf[RT].
//
// This wave's share of sum q c of the workgroup's RT x IMG::T accumulator tiles
// and of the row sums, handed to tail(acc, rs) -- as decode8qg_body hands its
// sums on.  The accumulators are the function's own: as arrays of the kernel
// filled through references, the RT T = 8 forms kept them in memory (up to
// 372 B of scratch a lane and 285 spilled VGPRs in the first version).
template <int RT, bool ALIGNED, typename IMG, typename Tail>
__device__ __forceinline__ void decode8r_body(const int8_t* __restrict__ X, const IMG& img, int K, int M, int nkb,
                                             int ntiles, int t0, int wave, int lane, Tail tail) {
    constexpr int T = IMG::T;
    i32x4 acc[RT][T], rs[RT];
    static_assert(RT >= 2 && RT * T <= kDecRowsAcc, "all row tiles' sums at once in 64 KiB");
    const int xr = lane & 15, kq = lane >> 4;
    bool row_ok[RT];
    const int8_t* xrow[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        row_ok[rt] = 16 * rt + xr < M;
        xrow[rt] = X + (size_t)(row_ok[rt] ? 16 * rt + xr : 0) * K;
    }

    const u32x4* wp[T];
    img.ptrs(t0, ntiles, nkb, lane, wp);

    constexpr int H = RT > 2 ? 2 : 4;  // steps of an X batch
    auto load_x = [&](int kb, int batch, i32x4 (&xf)[RT][H]) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int ii = 0; ii < H; ++ii) {
                const int k = kW2Blk * kb + 64 * (H * batch + ii) + 16 * kq;
                xf[rt][ii] = i32x4{0, 0, 0, 0};
                if constexpr (ALIGNED) {
                    if (row_ok[rt] && k < K) xf[rt][ii] = *reinterpret_cast<const i32x4*>(xrow[rt] + k);
                } else {
                    if (row_ok[rt] && k < K) {
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const uint32_t b = k + j < K ? (uint32_t)(uint8_t)xrow[rt][k + j] : 0u;
                            xf[rt][ii][j >> 2] |= (int)(b << (8 * (j & 3)));
                        }
                    }
                }
            }
        }
    };

#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        rs[rt] = i32x4{0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < T; ++t) acc[rt][t] = i32x4{0, 0, 0, 0};
    }

    i32x4 xa[RT][H], xb[RT][H];
    u32x4 pa[T], pb[T];
    int kb = wave;
    if (kb < nkb) {
        decode_load_w<T>(wp, kb, pa);
        load_x(kb, 0, xa);
    }
    while (kb < nkb) {  // uniform
        int nx = kb + kDecWaves;
        if constexpr (H == 4) {  // two blocks a round: a's, then b's
            if (nx < nkb) {
                decode_load_w<T>(wp, nx, pb);
                load_x(nx, 0, xb);
            }
            decode_steps_rows<RT, T, 4, 0>(xa, pa, M, acc, rs);
            kb = nx;
            if (kb >= nkb) break;
            nx = kb + kDecWaves;
            if (nx < nkb) {
                decode_load_w<T>(wp, nx, pa);
                load_x(nx, 0, xa);
            }
            decode_steps_rows<RT, T, 4, 0>(xb, pb, M, acc, rs);
        } else {  // one block a round: its first half in a, its second in b
            load_x(kb, 1, xb);
            if (nx < nkb) decode_load_w<T>(wp, nx, pb);
            decode_steps_rows<RT, T, 2, 0>(xa, pa, M, acc, rs);
            if (nx < nkb) load_x(nx, 0, xa);
            decode_steps_rows<RT, T, 2, 1>(xb, pa, M, acc, rs);
#pragma unroll
            for (int t = 0; t < T; ++t) pa[t] = pb[t];
        }
        kb = nx;
    }
    tail(acc, rs);
}

// decode_reduce_store_glu over RT row tiles: `red` holds WAVES x RT x 2 TG
// accumulator tiles, of each row tile the TG gate tiles and then the TG up
// tiles; row r of tile rt is row 16 rt + r of Y.  One thread per output adds the
// WAVES shares of Sg and of Su, applies i8_out to each and i8_glu to the pair,
// and does the one store.  Every thread of the workgroup calls this.
template <int WAVES, int RT, int TG, typename TY>
__device__ __forceinline__ void decode_reduce_store_glu_rows(int* red, const i32x4 (&acc)[RT][2 * TG],
                                                             const i32x4 (&rs)[RT], int wave, int lane, int t0, int M,
                                                             int N, const float* __restrict__ scale, const GluEpi& e,
                                                             TY* __restrict__ Y, int ldy) {
    constexpr int T = 2 * TG;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[((wave * RT + rt) * T + t) * 256 + r * 64 + lane] = acc[rt][t][r] - rs[rt][r];
    __syncthreads();
    for (int o = threadIdx.x; o < RT * TG * 256; o += WAVES * 64) {
        const int row = o / (16 * TG), cg = o % (16 * TG), t = cg >> 4, c = cg & 15;
        const int col = (t0 + t) * kW2Cols + c;
        if (row >= M || col >= N) continue;
        const int rt = row >> 4, r = row & 15;
        int Sg = 0, Su = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            Sg += red[((w * RT + rt) * T + t) * 256 + (r & 3) * 64 + (r >> 2) * 16 + c];
            Su += red[((w * RT + rt) * T + TG + t) * 256 + (r & 3) * 64 + (r >> 2) * 16 + c];
        }
        const float s = scale ? scale[row] : 1.0f;
        const float g = i8_out<false>(Sg, s, i8_cscale(e.cg, col), e.bg[col], 0.0f);
        const float u = i8_out<false>(Su, s, i8_cscale(e.cu, col), e.bu[col], 0.0f);
        I8Y<TY>::put(Y + (size_t)row * ldy + col, i8_glu(g, u, e.act));
    }
}

// The gated k_decode8r; act is a uniform branch in the tail.
template <int RT, int TG, bool ALIGNED, typename TY>
__global__ void __launch_bounds__(kDecWaves * 64) k_decode8gr(const int8_t* __restrict__ X,
                                                               const uint32_t* __restrict__ Wg,
                                                               const uint32_t* __restrict__ Wu, int K, int M, int N,
                                                               int nkb, int ntiles, const float* __restrict__ scale,
                                                               GluEpi e, TY* __restrict__ Y, int ldy) {
    __shared__ int red[kDecWaves * RT * 2 * TG * 256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = blockIdx.x * TG;
    decode8r_body<RT, ALIGNED>(X, DecodeImg2<TG>{Wg, Wu}, K, M, nkb, ntiles, t0, wave, lane,
                               [&](const i32x4(&acc)[RT][2 * TG], const i32x4(&rs)[RT]) {
                                   decode_reduce_store_glu_rows<kDecWaves, RT, TG>(red, acc, rs, wave, lane, t0, M, N, scale,
                                                                                   e, Y, ldy);
                               });
}

// The grouped k_decode8r: k_decode8m's grid and member table.
template <int RT, int T, bool ALIGNED, typename TY>
__global__ void __launch_bounds__(kDecWaves * 64) k_decode8mr(const int8_t* __restrict__ X, GroupTable g, int K, int M,
                                                               int nkb, const float* __restrict__ scale) {
    __shared__ int red[kDecWaves * RT * T * 256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const GroupSlot s = decode_group_slot(g, blockIdx.x);
    const int t0 = (blockIdx.x - s.first) * T;  // in the member's own tiles
    decode8r_body<RT, ALIGNED>(X, DecodeImg1<T>{s.W2, 0}, K, M, nkb, s.ntiles, t0, wave, lane,
                               [&](const i32x4(&acc)[RT][T], const i32x4(&rs)[RT]) {
                                   decode_reduce_store_rows<kDecWaves, RT, T, false, false, TY>(
                                       red, acc, rs, wave, lane, t0, M, s.N, scale, s.cscale, s.bias, static_cast<TY*>(s.Y),
                                       s.ldy, 0.0f, nullptr, 0);
                               });
}

}  // namespace

hipError_t decode_build_w2(const int8_t* w8, int ncols, int K, int ld8, uint32_t* w2, int* bad, hipStream_t st) {
    if (ncols <= 0 || K <= 0 || ld8 < K || ld8 % 16) return hipErrorInvalidValue;
    const int nkb = w2_kblocks(K);
    const size_t dwords = w2_image_bytes(K, ncols) / 4;
    const size_t blocks = (dwords + 255) / 256;
    hipLaunchKernelGGL(k_w2_from, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, w8, ncols, K, ld8,
                       nkb, dwords, w2, bad);
    return hipGetLastError();
}

hipError_t w2_from_tcsc(const int* csp, const int* csn, const int* rip, const int* rin, int col_begin, int ncols, int K,
                        uint32_t* w2, int* bad, hipStream_t st) {
    if (ncols <= 0 || K <= 0 || K >= kDecodeMaxK || col_begin < 0 || !csp || !csn || !w2 || !bad)
        return hipErrorInvalidValue;
    const int nkb = w2_kblocks(K), nkg = (nkb + kW2BuildKb - 1) / kW2BuildKb;
    const long long blocks = (long long)w2_col_tiles(ncols) * nkg;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_w2_from_tcsc, dim3((unsigned)blocks), dim3(256), 0, st, csp, csn, rip, rin, col_begin, ncols, K,
                       nkb, nkg, w2, bad);
    return hipGetLastError();
}

hipError_t w2_check(const uint32_t* w2, int ncols, int K, unsigned long long* counts, int* bad, hipStream_t st) {
    if (ncols <= 0 || K <= 0 || K >= kDecodeMaxK || !w2 || !counts || !bad) return hipErrorInvalidValue;
    const size_t dwords = w2_image_bytes(K, ncols) / 4;
    const size_t blocks = (dwords + 255) / 256;
    hipLaunchKernelGGL(k_w2_check, dim3((unsigned)(blocks < kW2CheckBlocks ? blocks : kW2CheckBlocks)), dim3(256), 0, st, w2, ncols, K,
                       w2_kblocks(K), dwords, counts, bad);
    return hipGetLastError();
}

bool w2_unpack_fits(int ncols, int K) {
    const long long nkb = w2_kblocks(K);
    return (long long)w2_col_tiles(ncols) * nkb <= 0x7fffffffLL && (long long)ncols * nkb + 1 <= 0x7fffffffLL;
}

hipError_t w2_unpack_counts(const uint32_t* w2, int ncols, int K, int* cntp, int* cntn, hipStream_t st) {
    if (ncols <= 0 || K <= 0 || K >= kDecodeMaxK || !w2_unpack_fits(ncols, K) || !w2 || !cntp || !cntn)
        return hipErrorInvalidValue;
    const int nkb = w2_kblocks(K);
    hipLaunchKernelGGL(k_w2_unpack<false>, dim3((unsigned)(w2_col_tiles(ncols) * nkb)), dim3(256), 0, st, w2, ncols, K,
                       nkb, cntp, cntn, nullptr, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t w2_unpack_col_start(const int* offp, const int* offn, int ncols, int K, int* csp, int* csn, hipStream_t st) {
    if (ncols <= 0 || K <= 0 || !offp || !offn || !csp || !csn) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_w2_col_start, dim3((unsigned)(ncols / 256 + 1)), dim3(256), 0, st, offp, offn, ncols,
                       w2_kblocks(K), csp, csn);
    return hipGetLastError();
}

hipError_t w2_unpack_fill(const uint32_t* w2, int ncols, int K, const int* offp, const int* offn, int* rip, int* rin,
                          hipStream_t st) {
    if (ncols <= 0 || K <= 0 || K >= kDecodeMaxK || !w2_unpack_fits(ncols, K) || !w2 || !offp || !offn || !rip || !rin)
        return hipErrorInvalidValue;
    const int nkb = w2_kblocks(K);
    hipLaunchKernelGGL(k_w2_unpack<true>, dim3((unsigned)(w2_col_tiles(ncols) * nkb)), dim3(256), 0, st, w2, ncols, K,
                       nkb, nullptr, nullptr, offp, offn, rip, rin);
    return hipGetLastError();
}

// Column tiles per workgroup.  A workgroup reads all of X (M K bytes, from the
// L2) and 4 T K bytes of image (from HBM): T >= M / 4 keeps the first at or
// below the second.  But T tiles per workgroup leave ceil(tiles / T)
// workgroups, and below one per CU the stream has too few loads in flight, so
// T is halved until the grid covers the chip (or T = 1).
int decode_tiles_per_wg(int M, int N, int num_cus) {
    if (kDecTiles) return kDecTiles;
    const int ntiles = w2_col_tiles(N), cus = num_cus > 0 ? num_cus : 256;
    int T = M > 8 ? 4 : M > 4 ? 2 : 1;
    while (T > 1 && (ntiles + T - 1) / T < cus) T >>= 1;
    return T;
}

// Row tiles and column tiles per workgroup of a launch of 17 .. 64 rows
// (k_decode8r).  RT: two 16-row tiles up to 32 rows, four above
// (at 33 .. 48 rows the fourth issues no MFMA).  T: a workgroup reads all of X
// from the L2 whatever T is, so the launch's X traffic falls as 1 / T and the
// rule starts from the most the LDS holds, RT T = 8 (kDecRowsAcc); the other constraint is
// decode_tiles_per_wg's -- below one workgroup per CU the stream of the image
// has too few loads in flight -- so T is halved until the grid covers the chip
// (or T = 1).
int decode_row_tiles(int M) { return M <= kDecodeMaxM ? 1 : M <= 32 ? 2 : 4; }
int decode_rows_tiles_per_wg(int M, int N, int num_cus) {
    const int ntiles = w2_col_tiles(N), cus = num_cus > 0 ? num_cus : 256;
    int T = kDecRowsAcc / decode_row_tiles(M);
    if (kDecRowsTiles) return kDecRowsTiles < T ? kDecRowsTiles : T;
    while (T > 1 && (ntiles + T - 1) / T < cus) T >>= 1;
    return T;
}

// The one decode launch (tcsc_internal.h).  Everything a kernel is instantiated
// over -- Y type, tiles per workgroup, ALIGNED, PRELU or the residual (§26: the
// two exclude each other), and for an X the launch quantizes its type and the
// norm -- becomes a template argument here and nowhere else; x and e are
// unpacked into the kernels' parameter lists.  Above 16 rows (§27) the kernel is
// k_decode8r over (RT, T) in {(2, 4), (2, 2), (2, 1), (4, 2), (4, 1)}, on an int8 X
// alone: the forms that quantize inside are not extended.
hipError_t decode_gemm(const DecodeX& x, const uint32_t* w2, int K, int M, int N, const I8Epi& e, int num_cus,
                       hipStream_t st) {
    const bool quant = x.xtype != kI8;
    if (M < 1 || M > kDecodeRowsMax || (quant && M > kDecodeMaxM) || K < 1 || K >= kDecodeMaxK || N < 1 || !x.X || !w2 ||
        (quant && !x.scale_out) || !e.B || !e.y.Y || e.ldy < N ||
        (e.R && (e.prelu || e.ldr < N || (e.R == e.y.Y && e.ldr != e.ldy))))
        return hipErrorInvalidValue;
    const int rtiles = decode_row_tiles(M);
    const int ntiles = w2_col_tiles(N), nkb = w2_kblocks(K);
    const int tiles = rtiles > 1 ? decode_rows_tiles_per_wg(M, N, num_cus) : decode_tiles_per_wg(M, N, num_cus);
    const dim3 grid((ntiles + tiles - 1) / tiles);
    const bool aligned = x.xtype == kI8    ? XSrc<int8_t>::vec_ok(static_cast<const int8_t*>(x.X), K)
                         : x.xtype == kBf16 ? XSrc<uint16_t>::vec_ok(static_cast<const uint16_t*>(x.X), K)
                                            : XSrc<float>::vec_ok(static_cast<const float*>(x.X), K);
    auto with_tiles = [&](auto&& f) {
        if (tiles == 4) return f(std::integral_constant<int, 4>{});
        if (tiles == 2) return f(std::integral_constant<int, 2>{});
        return f(std::integral_constant<int, 1>{});
    };
    // the tail: 0 plain, 1 PReLU, 2 the residual
    auto with_tail = [&](auto&& f) {
        if (e.R) return f(std::integral_constant<int, 2>{});
        if (e.prelu) return f(std::integral_constant<int, 1>{});
        return f(std::integral_constant<int, 0>{});
    };
    if (rtiles > 1) {
        with_elem(e.y.ytype == kYBf16, [&](auto ty) {
            using TY = typename decltype(ty)::type;
            TY* Y = static_cast<TY*>(e.y.Y);
            const TY* R = static_cast<const TY*>(e.R);
            with_tiles([&](auto t) {
                with_bool(aligned, [&](auto al) {
                    with_tail([&](auto tl) {
                        with_bool(rtiles == 4, [&](auto r4) {
                            constexpr int T = decltype(t)::value, RT = decltype(r4)::value ? 4 : 2;
                            constexpr bool AL = decltype(al)::value, PR = decltype(tl)::value == 1,
                                           RS = decltype(tl)::value == 2;
                            if constexpr (RT * T <= kDecRowsAcc)  // the rule never asks for more
                                hipLaunchKernelGGL((k_decode8r<RT, T, AL, PR, TY, RS>), grid, dim3(kDecWaves * 64), 0, st,
                                                   static_cast<const int8_t*>(x.X), w2, K, M, N, nkb, ntiles, e.rscale,
                                                   e.y.cscale, e.B, Y, e.ldy, e.a, R, e.ldr);
                        });
                    });
                });
            });
        });
        return hipGetLastError();
    }
    with_elem(e.y.ytype == kYBf16, [&](auto ty) {
        using TY = typename decltype(ty)::type;
        TY* Y = static_cast<TY*>(e.y.Y);
        const TY* R = static_cast<const TY*>(e.R);
        with_tiles([&](auto t) {
            with_bool(aligned, [&](auto al) {
                with_tail([&](auto tl) {
                    constexpr int T = decltype(t)::value;
                    constexpr bool AL = decltype(al)::value, PR = decltype(tl)::value == 1, RS = decltype(tl)::value == 2;
                    if (!quant) {
                        hipLaunchKernelGGL((k_decode8<T, AL, PR, TY, RS>), grid, dim3(kDecWaves * 64), 0, st,
                                           static_cast<const int8_t*>(x.X), w2, K, M, N, nkb, ntiles, e.rscale, e.y.cscale,
                                           e.B, Y, e.ldy, e.a, R, e.ldr);
                        return;
                    }
                    with_elem(x.xtype == kBf16, [&](auto tx) {
                        using TX = typename decltype(tx)::type;
                        with_bool(x.norm != nullptr, [&](auto nm) {
                            hipLaunchKernelGGL((k_decode8q<TX, T, AL, PR, TY, decltype(nm)::value, RS>), grid,
                                               dim3(kQWaves * 64), 0, st, static_cast<const TX*>(x.X), w2, K, M, N, nkb,
                                               ntiles, x.scale_out, e.y.cscale, e.B, Y, e.ldy, e.a,
                                               x.norm ? x.norm->gamma : nullptr, x.norm ? x.norm->eps : 0.0f, R, e.ldr);
                        });
                    });
                });
            });
        });
    });
    return hipGetLastError();
}

// Column tiles per workgroup of a gated launch: decode_tiles_per_wg's rule on
// the 2 TG image tiles the workgroup streams (a workgroup holds at most four),
// the grid being its ceil(tiles / TG) workgroups.
int decode_glu_tiles_per_wg(int M, int N, int num_cus) {
    if (kDecTiles) return kDecTiles == 4 ? 2 : 1;
    const int ntiles = w2_col_tiles(N), cus = num_cus > 0 ? num_cus : 256;
    int T = M > 8 ? 4 : 2;  // the rule's 1 is below one tile of each image
    while (T > 2 && (ntiles + T / 2 - 1) / (T / 2) < cus) T >>= 1;
    return T / 2;
}

// Column tiles per workgroup of a gated launch of 17 .. 64 rows (k_decode8gr,
// DESIGN.md §28): decode_rows_tiles_per_wg's rule on the 2 TG image tiles the
// workgroup streams -- from the most the accumulators allow, RT 2 TG = 8
// (kDecRowsAcc), halved while the grid of ceil(tiles / TG) workgroups is below
// the CU count, down to TG = 1.
int decode_glu_rows_tiles_per_wg(int M, int N, int num_cus) {
    const int ntiles = w2_col_tiles(N), cus = num_cus > 0 ? num_cus : 256;
    int TG = kDecRowsAcc / (2 * decode_row_tiles(M));
    if (kDecRowsTiles) return kDecRowsTiles >= 2 * TG ? TG : kDecRowsTiles > 1 ? kDecRowsTiles / 2 : 1;
    while (TG > 1 && (ntiles + TG - 1) / TG < cus) TG >>= 1;
    return TG;
}

// The gated decode launch (tcsc_internal.h): decode_gemm's dispatch without the
// PReLU axis and over TG in {1, 2}; the activation is a kernel argument.  Above
// 16 rows (§28) the kernel is k_decode8gr over (RT, TG) in {(2, 2), (2, 1), (4, 1)},
// on an int8 X alone.
hipError_t decode_glu(const DecodeX& x, const uint32_t* wg, const uint32_t* wu, int K, int M, int N, const I8Epi& gate,
                      const I8Epi& up, int num_cus, hipStream_t st) {
    const bool quant = x.xtype != kI8;
    if (M < 1 || M > kDecodeRowsMax || (quant && M > kDecodeMaxM) || K < 1 || K >= kDecodeMaxK || N < 1 || !x.X || !wg || !wu || (quant && !x.scale_out) ||
        !gate.B || !up.B || !up.y.Y || up.ldy < N || (up.act != kGluRelu2 && up.act != kGluSilu))
        return hipErrorInvalidValue;
    const int rtiles = decode_row_tiles(M);
    const int ntiles = w2_col_tiles(N), nkb = w2_kblocks(K);
    const int tiles = rtiles > 1 ? decode_glu_rows_tiles_per_wg(M, N, num_cus) : decode_glu_tiles_per_wg(M, N, num_cus);
    const dim3 grid((ntiles + tiles - 1) / tiles);
    const bool aligned = x.xtype == kI8    ? XSrc<int8_t>::vec_ok(static_cast<const int8_t*>(x.X), K)
                         : x.xtype == kBf16 ? XSrc<uint16_t>::vec_ok(static_cast<const uint16_t*>(x.X), K)
                                            : XSrc<float>::vec_ok(static_cast<const float*>(x.X), K);
    const GluEpi e{gate.y.cscale, gate.B, up.y.cscale, up.B, up.act};
    if (rtiles > 1) {
        with_elem(up.y.ytype == kYBf16, [&](auto ty) {
            using TY = typename decltype(ty)::type;
            TY* Y = static_cast<TY*>(up.y.Y);
            with_bool(tiles == 2, [&](auto t2) {
                with_bool(aligned, [&](auto al) {
                    with_bool(rtiles == 4, [&](auto r4) {
                        constexpr int TG = decltype(t2)::value ? 2 : 1, RT = decltype(r4)::value ? 4 : 2;
                        constexpr bool AL = decltype(al)::value;
                        if constexpr (RT * 2 * TG <= kDecRowsAcc)  // the rule never asks for more
                            hipLaunchKernelGGL((k_decode8gr<RT, TG, AL, TY>), grid, dim3(kDecWaves * 64), 0, st,
                                               static_cast<const int8_t*>(x.X), wg, wu, K, M, N, nkb, ntiles, up.rscale, e,
                                               Y, up.ldy);
                    });
                });
            });
        });
        return hipGetLastError();
    }
    with_elem(up.y.ytype == kYBf16, [&](auto ty) {
        using TY = typename decltype(ty)::type;
        TY* Y = static_cast<TY*>(up.y.Y);
        with_bool(tiles == 2, [&](auto t2) {
            with_bool(aligned, [&](auto al) {
                constexpr int TG = decltype(t2)::value ? 2 : 1;
                constexpr bool AL = decltype(al)::value;
                if (!quant) {
                    hipLaunchKernelGGL((k_decode8g<TG, AL, TY>), grid, dim3(kDecWaves * 64), 0, st,
                                       static_cast<const int8_t*>(x.X), wg, wu, K, M, N, nkb, ntiles, up.rscale, e, Y,
                                       up.ldy);
                    return;
                }
                with_elem(x.xtype == kBf16, [&](auto tx) {
                    using TX = typename decltype(tx)::type;
                    with_bool(x.norm != nullptr, [&](auto nm) {
                        hipLaunchKernelGGL((k_decode8qg<TX, TG, AL, TY, decltype(nm)::value>), grid, dim3(kQWaves * 64),
                                           0, st, static_cast<const TX*>(x.X), wg, wu, K, M, N, nkb, ntiles, x.scale_out,
                                           e, Y, up.ldy, x.norm ? x.norm->gamma : nullptr, x.norm ? x.norm->eps : 0.0f);
                    });
                });
            });
        });
    });
    return hipGetLastError();
}

// Column tiles per workgroup of a grouped launch, one value for all members:
// decode_tiles_per_wg's rule on the whole grid, the sum of the members'
// ceil(tiles_i / T) workgroups.  One member: decode_tiles_per_wg itself.
long long decode_group_wgs(const int* cols, int count, int T) {
    long long w = 0;
    for (int i = 0; i < count; ++i) w += (w2_col_tiles(cols[i]) + T - 1) / T;
    return w;
}
int decode_group_tiles_per_wg(int M, const int* cols, int count, int num_cus) {
    if (kDecTiles) return kDecTiles;
    const int cus = num_cus > 0 ? num_cus : 256;
    int T = M > 8 ? 4 : M > 4 ? 2 : 1;
    while (T > 1 && decode_group_wgs(cols, count, T) < cus) T >>= 1;
    return T;
}

// The one T of a grouped launch of 17 .. 64 rows (k_decode8mr):
// decode_rows_tiles_per_wg's rule -- from RT T = 8 (kDecRowsAcc) down to T = 1
// -- tested against the whole concatenated grid.
int decode_group_rows_tiles_per_wg(int M, const int* cols, int count, int num_cus) {
    const int cus = num_cus > 0 ? num_cus : 256;
    int T = kDecRowsAcc / decode_row_tiles(M);
    if (kDecRowsTiles) return kDecRowsTiles < T ? kDecRowsTiles : T;
    while (T > 1 && decode_group_wgs(cols, count, T) < cus) T >>= 1;
    return T;
}

// The grouped decode launch (tcsc_internal.h): decode_gemm's dispatch without
// the PReLU and norm axes; the members travel as one table by value.  Above 16
// rows (§28) the kernel is k_decode8mr over (RT, T) in {(2, 4), (2, 2), (2, 1),
// (4, 2), (4, 1)}, on an int8 X alone.
hipError_t decode_group(const DecodeX& x, const DecodeMember* m, int count, int K, int M, int num_cus, hipStream_t st) {
    const bool quant = x.xtype != kI8;
    if (M < 1 || M > kDecodeRowsMax || (quant && M > kDecodeMaxM) || K < 1 || K >= kDecodeMaxK || count < 1 || count > kGroupMax || !m || !x.X ||
        (quant && !x.scale_out) || x.norm)
        return hipErrorInvalidValue;
    int cols[kGroupMax];
    for (int i = 0; i < count; ++i) {
        if (m[i].N < 1 || !m[i].w2 || !m[i].e.B || !m[i].e.y.Y || m[i].e.ldy < m[i].N || m[i].e.y.ytype != m[0].e.y.ytype ||
            m[i].e.prelu)
            return hipErrorInvalidValue;
        cols[i] = m[i].N;
    }
    const int rtiles = decode_row_tiles(M);
    const int nkb = w2_kblocks(K), tiles = rtiles > 1 ? decode_group_rows_tiles_per_wg(M, cols, count, num_cus)
                                                      : decode_group_tiles_per_wg(M, cols, count, num_cus);
    const long long wgs = decode_group_wgs(cols, count, tiles);
    if (wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    GroupTable g{};
    int first = 0;
    for (int i = 0; i < kGroupMax; ++i) {
        g.m[i].first = 0x7fffffff;  // a slot past the group: no block is at or beyond it
        if (i >= count) continue;
        const int ntiles = w2_col_tiles(m[i].N);
        g.m[i] = GroupSlot{m[i].w2, m[i].e.y.cscale, m[i].e.B, m[i].e.y.Y, m[i].N, ntiles, m[i].e.ldy, first};
        first += (ntiles + tiles - 1) / tiles;
    }
    const dim3 grid((unsigned)wgs);
    const bool aligned = x.xtype == kI8    ? XSrc<int8_t>::vec_ok(static_cast<const int8_t*>(x.X), K)
                         : x.xtype == kBf16 ? XSrc<uint16_t>::vec_ok(static_cast<const uint16_t*>(x.X), K)
                                            : XSrc<float>::vec_ok(static_cast<const float*>(x.X), K);
    auto with_tiles = [&](auto&& f) {
        if (tiles == 4) return f(std::integral_constant<int, 4>{});
        if (tiles == 2) return f(std::integral_constant<int, 2>{});
        return f(std::integral_constant<int, 1>{});
    };
    if (rtiles > 1) {
        with_elem(m[0].e.y.ytype == kYBf16, [&](auto ty) {
            using TY = typename decltype(ty)::type;
            with_tiles([&](auto t) {
                with_bool(aligned, [&](auto al) {
                    with_bool(rtiles == 4, [&](auto r4) {
                        constexpr int T = decltype(t)::value, RT = decltype(r4)::value ? 4 : 2;
                        constexpr bool AL = decltype(al)::value;
                        if constexpr (RT * T <= kDecRowsAcc)  // the rule never asks for more
                            hipLaunchKernelGGL((k_decode8mr<RT, T, AL, TY>), grid, dim3(kDecWaves * 64), 0, st,
                                               static_cast<const int8_t*>(x.X), g, K, M, nkb, m[0].e.rscale);
                    });
                });
            });
        });
        return hipGetLastError();
    }
    with_elem(m[0].e.y.ytype == kYBf16, [&](auto ty) {
        using TY = typename decltype(ty)::type;
        with_tiles([&](auto t) {
            with_bool(aligned, [&](auto al) {
                constexpr int T = decltype(t)::value;
                constexpr bool AL = decltype(al)::value;
                if (!quant) {
                    hipLaunchKernelGGL((k_decode8m<T, AL, TY>), grid, dim3(kDecWaves * 64), 0, st,
                                       static_cast<const int8_t*>(x.X), g, K, M, nkb, m[0].e.rscale);
                    return;
                }
                with_elem(x.xtype == kBf16, [&](auto tx) {
                    using TX = typename decltype(tx)::type;
                    hipLaunchKernelGGL((k_decode8qm<TX, T, AL, TY>), grid, dim3(kQWaves * 64), 0, st,
                                       static_cast<const TX*>(x.X), g, K, M, nkb, x.scale_out);
                });
            });
        });
    });
    return hipGetLastError();
}

}  // namespace tcsc
