// tcsc_wide.hip -- the second geometry of kernel K1: 16 waves x 22 columns
// = 352 output columns per workgroup (DESIGN.md §4 "Two geometries").
//
// k_stream (tcsc_kernels.hip) gives every wave 16 columns: a workgroup covers
// 256 columns and stages one 48-KiB X^T chunk for them.  At the headline shape
// (M = 4096, N = 16384 on 256 CUs) that is 64 column blocks x 16 row tiles =
// 1024 workgroups, four rounds of the chip, and the chunk period sits on the
// L2 -> LDS staging time.  With 22 columns per wave the same shape is 47 x 16
// = 752 workgroups, three rounds, and 27 % fewer staged bytes.  The launcher
// takes this kernel only where a rounds model says it pays (wide_pays,
// tcsc_api.cpp); everything else -- split K, the reference orders, the
// combines, the backward plans -- stays on the 16-column kernel.
//
// Same arithmetic as k_stream<.., OUT 0, ORDER 0>: every column's nonzeros
// are added in ascending k, the bias last (or first), so the output bits are
// those of the 16-column kernel.  What differs:
//  * the generated loop (gather_asm_w22.inc: cw 22, batch 3, cap 30 -- 88
//    accumulator and 24 X registers; batch 4 leaves 8 registers for everything
//    else, below what the generator accepts.  A wave's chunk stream averages
//    21 entries at the headline density, so the scalar buffer holds 30: with
//    24, one wave in four reloads it in every chunk, and the whole workgroup
//    waits for that exposed scalar load at the next barrier -- measured 5 %
//    of the kernel);
//  * the LDS-DMA keeps one per-lane offset (16 * lane) and moves the per-row
//    source offset into the 64-bit scalar base (two SALU per row on the four
//    DMA waves) instead of twelve per-lane offsets;
//  * the chunk loop has only s0..s35 beside the gather's pinned SGPRs, so the
//    epilogue reads its arguments and recomputes its tile after the loop;
//  * which 22 of a column block's 352 columns a wave owns is a plan-time
//    choice, the slot map wperm[block][16 * 22] (k_wide_balance: the busiest
//    wave ends every chunk, so the columns are dealt to level the waves'
//    entries per chunk).  The chunk loop does not know: only the streams
//    (wide_counts / wide_fill) and the epilogue's parking read the map;
//  * the epilogue parks each slot's column with 4-byte LDS stores at the
//    map's position in rows of 1408 + 16 bytes and stores each tile row as
//    88 quads;
//  * the streams are re-grouped from the plan's 16-column streams on the
//    device (wide_counts / wide_fill), so a plan needs nothing but its own
//    arrays to grow the second copy.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "tcsc_internal.h"

namespace tcsc {

#include "gather_asm_w22.inc"

static_assert(TCSCW_GEN_CW == kWideCW && TCSCW_GEN_BATCH == kWideBatch, "generated loop geometry");
static_assert(TCSCW_GEN_CAP + kHdr <= kEntGuard, "stream prefetch stays inside the entry guard");
static_assert(TCSCW_GEN_HDR == 2 * kHdr, "generated loop and plan agree on the chunk header");
static_assert(TCSCW_GEN_BUDGET == (512 / kWavesPerSimd) / 8 * 8, "generated loop VGPR budget");
static_assert(TCSCW_GEN_TAIL == 1, "the wide streams are unpadded");
static_assert(TCSCW_GEN_TOUCH == 0 && TCSCW_GEN_PF == 0, "no scalar-cache touches in the wide loop");
static_assert(4 * kWideCW <= 255, "slot index must fit the 8-bit gpr_idx field");
static_assert(kWaves == 16 && kTK % 16 == 0 && kNBuf >= 3, "the wide kernel's DMA split and ring");

namespace {

// the accumulator registers, in the generated asm operands' tuples
typedef float f32x32_t __attribute__((ext_vector_type(32)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x8_t __attribute__((ext_vector_type(8)));
constexpr int kAccWidths[] = {TCSCW_ACC_WIDTHS};
static_assert(sizeof(kAccWidths) == 4 * sizeof(int) && kAccWidths[0] == 32 && kAccWidths[1] == 32 &&
                  kAccWidths[2] == 16 && kAccWidths[3] == 8,
              "AccW mirrors the generated operand tuples");
struct AccW {
    f32x32_t v0, v1;
    f32x16_t v2;
    f32x8_t v3;
};
// i is a compile-time constant after unrolling
__device__ __forceinline__ float acc_get(const AccW& a, int i) {
    return i < 32 ? a.v0[i] : i < 64 ? a.v1[i - 32] : i < 80 ? a.v2[i - 64] : a.v3[i - 80];
}
__device__ __forceinline__ void acc_set(AccW& a, int i, float v) {
    if (i < 32) a.v0[i] = v;
    else if (i < 64) a.v1[i - 32] = v;
    else if (i < 80) a.v2[i - 64] = v;
    else a.v3[i - 80] = v;
}
__device__ __forceinline__ void acc_zero(AccW& a) {
#pragma unroll
    for (int i = 0; i < 4 * kWideCW; ++i) acc_set(a, i, 0.f);
}

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(4))) const i32x16 const_i32x16;
typedef int sbuf_tail_t __attribute__((ext_vector_type(TCSCW_SBUF_TAIL ? TCSCW_SBUF_TAIL : 4)));
typedef __attribute__((address_space(4))) const sbuf_tail_t const_sbuf_tail;

// One chunk of this wave's stream (gather_stream of tcsc_kernels.hip, on the
// wide loop): header and first CAP entries already in the pinned SGPR buffer.
__device__ __forceinline__ void gather_stream_w(i32x16 (&sb)[TCSCW_SBUF_VECS], sbuf_tail_t& sbt,
                                                unsigned long long& ptr, unsigned lane16, unsigned mask, AccW& acc) {
    (void)sbt;
    unsigned m0sv;
    asm volatile(TCSCW_GATHER_ASM
                 : TCSCW_ACC_OPERANDS(acc), TCSCW_SBUF_OPERANDS(sb, sbt), TCSCW_PTR_OPERAND(ptr), [m0sv] "=&s"(m0sv)
                 : [lane] "v"(lane16), [mask] "v"(mask)
                 : TCSCW_GATHER_CLOBBERS);
}

__device__ __forceinline__ void load_stream_w(i32x16 (&sb)[TCSCW_SBUF_VECS], sbuf_tail_t& sbt, const char* p) {
    const_i32x16* q = reinterpret_cast<const_i32x16*>(reinterpret_cast<uintptr_t>(p));
#pragma unroll
    for (int i = 0; i < TCSCW_SBUF_VECS; ++i) sb[i] = q[i];
#if TCSCW_SBUF_TAIL
    sbt = *reinterpret_cast<const_sbuf_tail*>(reinterpret_cast<uintptr_t>(p + 64 * TCSCW_SBUF_VECS));
#endif
}

// LDS-DMA of one X^T chunk: wave w < kDmaWaves moves rows w*D .. w*D+D-1 (D =
// kDmaPerWave), two rows per M0 write.  Every lane's offset is 16 * lane; a
// row's source is the scalar base `row` + i * row_bytes, less the instruction
// offset (i % 2 KiB) that moves the LDS destination and the global source
// alike (dma_rows of tcsc_kernels.hip keeps that in twelve VGPRs instead).
struct DmaW {
    const char* next;     // this wave's first row of the next chunk, column m0
    unsigned lds_wave;    // LDS address of this wave's first row in buffer 0
    unsigned chunk_bytes;  // kTK * ldxt * 4 (a launch has at most 2^22 rows: below 2^32)
    unsigned row_bytes;    // ldxt * 4
};
static_assert(kDmaPerWave % 2 == 0, "whole pairs of DMA rows");

__device__ __forceinline__ void dma_next_chunk_w(DmaW& d, int buf, unsigned lane16) {
    const unsigned m0base = d.lds_wave + (unsigned)(buf * (kBufRows * kRowBytes));
    const char* row = d.next;
#pragma unroll
    for (int i0 = 0; i0 < kDmaPerWave; i0 += 2) {  // two rows per M0 write: two scalar bases live, not four
        const char* s0 = row;
        const char* s1 = row + (d.row_bytes - 1 * kRowBytes);
        unsigned sv;  // M0 is saved and restored around every statement that writes it
        asm volatile("s_mov_b32 %[sv], m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\t"
                     "global_load_lds_dwordx4 %2, %4 offset:1024\n\ts_mov_b32 m0, %[sv]"
                     : [sv] "=&s"(sv)
                     : "s"(m0base + i0 * kRowBytes), "v"(lane16), "s"(s0), "s"(s1)
                     : "memory");
        row += 2u * d.row_bytes;
    }
    d.next += d.chunk_bytes;
}
static_assert(kRowBytes == 1024, "the DMA's instruction offsets are whole 1-KiB rows");

__device__ __forceinline__ void pf_touch_w(unsigned m0, unsigned voff, const char* base) {
    unsigned sv;
    asm volatile("s_mov_b32 %[sv], m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %2, %3\n\t"
                 "s_mov_b32 m0, %[sv]"
                 : [sv] "=&s"(sv)
                 : "s"(m0), "v"(voff), "s"(base)
                 : "memory");
}

// XCD-aware tile order (xcd_tile of tcsc_kernels.hip, one K slice).
__device__ __forceinline__ void xcd_tile_w(int bx, int by, int ncb, int nrt, int& cb, int& rt) {
    const int T = ncb * nrt;
    const int L = bx + ncb * by;
    const int q = T >> 3, r = T & 7, x = L & 7;
    const int Lg = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (L >> 3);
    cb = Lg % ncb;
    rt = Lg / ncb;
}

constexpr int kEpiRowsW = 64;                         // tile rows per epilogue pass
constexpr int kStrideW = kWideWgCols * 4 + 16;        // bytes per parked tile row
constexpr int kLdsBytesW = kRingBytes + kPfScratch;
static_assert(kEpiRowsW * kStrideW <= kRingBytes, "the epilogue staging fits below the ring's end");
static_assert(kLdsBytesW <= 160 * 1024, "LDS");
static_assert(kWideCW <= 64 && kWideWgCols <= 65535, "one lane per slot reads its 16-bit column position");
static_assert(kWideWgCols % 4 == 0 && kWideWgCols / 4 > 64 && kWideWgCols / 4 <= 128,
              "a tile row is 64 quads plus a second, partial set");

}  // namespace

// The kernel's arguments as the kernarg segment lays them out (each at its
// natural alignment, in order).  The chunk loop has 36 SGPRs beside the 66 the
// gather pins (a 30-entry scalar buffer, header and chain pointer), so what
// only the epilogue needs (Bias, Y, wperm, ldy, a, M, ncols) is read from the
// kernarg segment after the loop instead of living in SGPRs across it.
struct WideArgs {
    const float* XT;
    const int2* ent;
    const int* sptr;
    const float* Bias;
    float* Y;
    const unsigned short* wperm;
    long long n_entries;
    int ldxt, M, G, ncols, nch, ldy;
    float a;
    int pf_dist, pf_lines;
};

template <bool BIAS_FIRST, bool PRELU>
__global__ void __launch_bounds__(kWaves * 64, kWavesPerSimd)
k_stream_w(const float* __restrict__ XT, const int2* __restrict__ ent, const int* __restrict__ sptr,
           const float* __restrict__ Bias0, float* __restrict__ Y0, const unsigned short* __restrict__ wperm0,
           long long n_entries, int ldxt, int M0, int G, int ncols0, int nch, int ldy0, float a0, int pf_dist,
           int pf_lines) {
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytesW];
    const int lane = threadIdx.x & 63;
    const unsigned lane16 = 16u * lane;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tcb, trt;
    xcd_tile_w(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y, tcb, trt);
    const int g = tcb * kWaves + wave;  // wave-column group
    const int m0 = trt * kTM;
    const bool active = g < G;

    AccW acc;
    acc_zero(acc);
    if (BIAS_FIRST && active) {
        // slot j's column through the slot map (the identity on a partial block: cb < ncols there)
        const int cb = lane < kWideCW ? tcb * kWideWgCols + wperm0[tcb * kWideWgCols + wave * kWideCW + lane] : ncols0;
        const float bv = cb < ncols0 ? Bias0[cb] : 0.f;
#pragma unroll
        for (int j = 0; j < kWideCW; ++j) {
            const float b = __shfl(bv, j);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc_set(acc, 4 * j + r, b);
        }
    }

    // the -0.0 pad row of every ring buffer (the guard entries point there)
    if (threadIdx.x < 64 * kNBuf) {
        const int b = threadIdx.x >> 6;
        reinterpret_cast<float4*>(lds + (b * kBufRows + kTK) * kRowBytes)[lane] = make_float4(-0.f, -0.f, -0.f, -0.f);
    }

    if (nch > 0) {
        // The chunk loop of k_stream's run_chain (ring of kNBuf, DMA issued by
        // the first kDmaWaves waves right after the barrier, one stream
        // prefetch per chunk): the same VMEM order per wave, so the same
        // top-of-chunk vmcnt.
        DmaW dma;
        dma.row_bytes = (unsigned)ldxt * 4u;
        dma.chunk_bytes = (unsigned)kTK * (unsigned)ldxt * 4u;
        dma.next = reinterpret_cast<const char*>(XT + m0) + (size_t)(wave * kDmaPerWave) * dma.row_bytes;
        dma.lds_wave = (unsigned)reinterpret_cast<uintptr_t>(lds) + (unsigned)(wave * kDmaPerWave * kRowBytes);
        const bool dma_wave = wave < kDmaWaves;  // uniform
        const unsigned pf_m0 = (unsigned)reinterpret_cast<uintptr_t>(lds) + kRingBytes + 256u * wave;
        const unsigned pf_s_off = (unsigned)pf_dist + 128u * (unsigned)(lane * pf_lines >> 6);
        auto pf_issue = [&](unsigned long long p) {
            if (kPfS) pf_touch_w(pf_m0, pf_s_off, reinterpret_cast<const char*>(p));
        };
        if (dma_wave) dma_next_chunk_w(dma, 0, lane16);  // DMA(0)
        unsigned long long cur =
            reinterpret_cast<unsigned long long>(ent + (active ? (long long)sptr[(long long)g * nch] : n_entries));
        i32x16 sb[TCSCW_SBUF_VECS];
        sbuf_tail_t sbt;
        load_stream_w(sb, sbt, reinterpret_cast<const char*>(cur));
        pf_issue(cur);
#pragma unroll
        for (int i = 1; i + 1 < kNBuf; ++i) {
            if (dma_wave) dma_next_chunk_w(dma, i % kNBuf, lane16);
            pf_issue(cur);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // pad rows
        const unsigned mask = 0x3ffu;
        int dbuf = kNBuf - 1;
        for (int c = 0; c < nch; ++c) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kNBuf - 2) * kDmaPerWave + (kPfS ? 2 : 0)) : "memory");
            __builtin_amdgcn_s_barrier();
            if (dma_wave) dma_next_chunk_w(dma, dbuf, lane16);  // DMA(c + kNBuf - 1) into the buffer chunk c-1 used
            gather_stream_w(sb, sbt, cur, lane16, mask, acc);   // leaves cur at the next chunk's header
            load_stream_w(sb, sbt, reinterpret_cast<const char*>(cur));
            pf_issue(cur);
            dbuf = dbuf == kNBuf - 1 ? 0 : dbuf + 1;
        }
        // no LDS-DMA may still be writing when the LDS is reused or released,
        // and the last (unused) stream load must have landed
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }

    // Epilogue (k_stream's, OUT 0 / HOW 0): per pass of 64 tile rows (every
    // fourth: lane l holds tile rows 4 l .. 4 l + 3) every wave parks its 64 x 22
    // block -- slot j at the column the slot map gives it, 4-byte stores -- then
    // each wave reads back whole parked rows (wave, wave + 16, ...) as 88 quads:
    // lane l stores quad l, lanes 0..23 also quad 64 + l.
    __syncthreads();  // every wave is done with the tile ring
    // the epilogue's arguments, read now (see WideArgs): the empty asm keeps the loads below it
    typedef __attribute__((address_space(4))) const WideArgs const_args;
    const_args* E = reinterpret_cast<const_args*>(reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr()));
    asm volatile("" : "+s"(E)::"memory");
    const float* __restrict__ Bias = E->Bias;
    float* __restrict__ Y = E->Y;
    const int M = E->M, ncols = E->ncols, ldy = E->ldy;
    const float a = E->a;
    // ... and the tile's coordinates, recomputed for the same reason (from laundered
    // workgroup ids, or the compiler reuses the values from before the loop)
    int bx = blockIdx.x, by = blockIdx.y, gx = gridDim.x, gy = gridDim.y;
    asm volatile("" : "+s"(bx), "+s"(by), "+s"(gx), "+s"(gy));
    const int wave_e = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tcb_e, trt_e;
    xcd_tile_w(bx, by, gx, gy, tcb_e, trt_e);
    const bool active_e = tcb_e * kWaves + wave_e < E->G;
    const int m0_e = trt_e * kTM;
    static_assert(kEpiRowsW == 64 && kTM == 4 * kEpiRowsW, "a pass parks one of each lane's four rows");
    constexpr int kQuads = kWideWgCols / 4;
    // this wave's 22 column positions in a parked row (the slot map): one 16-bit load per lane, uniform per slot
    const unsigned short* __restrict__ wperm = E->wperm;
    const int posv = lane < kWideCW ? wperm[tcb_e * kWideWgCols + wave_e * kWideCW + lane] : 0;
    int pos[kWideCW];
#pragma unroll
    for (int j = 0; j < kWideCW; ++j) pos[j] = __builtin_amdgcn_readlane(posv, j);
    const bool vec_ok = (ldy & 3) == 0 && ((reinterpret_cast<uintptr_t>(Y) & 15) == 0);
    float4 bq[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int col = tcb_e * kWideWgCols + 4 * (lane + 64 * s);
        const bool in = lane + 64 * s < kQuads;
        bq[s].x = (!BIAS_FIRST && in && col + 0 < ncols) ? Bias[col + 0] : 0.f;
        bq[s].y = (!BIAS_FIRST && in && col + 1 < ncols) ? Bias[col + 1] : 0.f;
        bq[s].z = (!BIAS_FIRST && in && col + 2 < ncols) ? Bias[col + 2] : 0.f;
        bq[s].w = (!BIAS_FIRST && in && col + 3 < ncols) ? Bias[col + 3] : 0.f;
    }
#pragma unroll
    for (int h = 0; h < kTM / kEpiRowsW; ++h) {
        // pass h: row h of every lane's four (tile row 4 * lane + h) into parked row `lane`, all 64 lanes
        // storing: 22 LDS stores per wave and pass
        if (active_e) {
#pragma unroll
            for (int j = 0; j < kWideCW; ++j)
                *reinterpret_cast<float*>(lds + lane * kStrideW + pos[j] * 4) = acc_get(acc, 4 * j + h);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kEpiRowsW / kWaves; ++i) {
            const int R = wave_e + kWaves * i;
            const int row = m0_e + 4 * R + h;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int q = lane + 64 * s;
                const int col = tcb_e * kWideWgCols + 4 * q;
                if (q < kQuads && row < M && col < ncols) {
                    float4 v = *reinterpret_cast<const float4*>(lds + R * kStrideW + q * 16);
                    if (!BIAS_FIRST) {
                        v.x += bq[s].x;
                        v.y += bq[s].y;
                        v.z += bq[s].z;
                        v.w += bq[s].w;
                    }
                    if (PRELU) {
                        v.x = (v.x < 0.0f) ? a * v.x : v.x;
                        v.y = (v.y < 0.0f) ? a * v.y : v.y;
                        v.z = (v.z < 0.0f) ? a * v.z : v.z;
                        v.w = (v.w < 0.0f) ? a * v.w : v.w;
                    }
                    float* dst = Y + (size_t)row * ldy + col;
                    if (vec_ok && col + 3 < ncols) {  // Y is never re-read here: keep it out of L2's way
                        typedef float nt4 __attribute__((ext_vector_type(4)));
                        nt4 w = {v.x, v.y, v.z, v.w};
                        __builtin_nontemporal_store(w, reinterpret_cast<nt4*>(dst));
                    } else {
                        dst[0] = v.x;
                        if (col + 1 < ncols) dst[1] = v.y;
                        if (col + 2 < ncols) dst[2] = v.z;
                        if (col + 3 < ncols) dst[3] = v.w;
                    }
                }
            }
        }
        if (h + 1 < kTM / kEpiRowsW) __syncthreads();  // region reused by the next pass
    }
}

// ---------------------------------------------------------------------------
// The wide streams from the plan's own 16-column streams
// ---------------------------------------------------------------------------
// A (group, chunk) stream lists its slots' columns one after the other, each
// column's entries in ascending k, so a 22-column stream is runs of entries
// of the 16-column streams of the same chunk that hold its columns (the slot
// map below says which), each run as it stands.  One thread walks one
// 16-column stream; only it touches the (chunk, column) cells of its group,
// so nothing is atomic.

namespace {

// entries of the stream of (g, c): [*first, *first + n); padding entries
// (padded 16-column streams only) point at the pad row and are skipped
__device__ __forceinline__ int stream_range(const int* __restrict__ sptr, long long i, int* first) {
    const int s0 = sptr[i], s1 = sptr[i + 1];
    *first = s0 + kHdr;
    return s1 - s0 - kHdr;
}
__device__ __forceinline__ bool is_pad(int word) { return ((word >> 10) % kBufRows) == kTK; }

// cnt[c*ncols + n] += entries of column n in chunk c (cnt zeroed by the caller)
__global__ void k_wide_col_counts(const int2* __restrict__ ent, const int* __restrict__ sptr, int G, int nch, int ncols,
                                  int* __restrict__ cnt) {
    const long long total = (long long)G * nch;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(i / nch), c = (int)(i % nch);
        int first;
        const int n = stream_range(sptr, i, &first);
        const int n0 = group_col0(g);
        int run = 0, slot = -1;
        for (int e = 0; e < n; ++e) {
            const int w = ent[first + e].y;
            if (is_pad(w)) continue;
            const int s = (w & 0x3ff) >> 2;
            if (s != slot) {
                if (run) cnt[(long long)c * ncols + n0 + slot] = run;
                slot = s;
                run = 0;
            }
            ++run;
        }
        if (run) cnt[(long long)c * ncols + n0 + slot] = run;
    }
}

// ---- the slot map ----------------------------------------------------------
// wperm[b * 352 + w * 22 + j] = the column (0..351, inside block b) that slot j
// of wave w owns; winv[col] = w * 22 + j, its inverse over the plan's columns.
// Every wave waits at the chunk barrier for the wave with the most entries in
// that chunk, so a block's cost is about sum_c max_w L[w][c], L[w][c] = the
// entries of wave w's columns in chunk c.  One workgroup per column block
// deals the block's columns to its 16 waves, heaviest column first (ties: the
// lower column), each to the wave with a free slot whose chunk profile it
// overlaps least: the smallest sum_c L[w][c] * cnt[c][col], in 64-bit integers,
// ties to the lowest wave.  Slots fill in that order.  The result is kept only
// where sum_c max_w L[w][c] is strictly below the contiguous assignment's; the
// last, partial block and every block under balance == 0 keep the identity.
// Integer arithmetic in a fixed order: the same W gives the same map.  L is
// 16 * nch ints per block in global memory (any number of chunks).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(kWaves * 64)
k_wide_balance(const int* __restrict__ cnt, int ncols, int nch, int balance, int* L0, unsigned short* __restrict__ wperm,
               unsigned short* __restrict__ winv) {
    __shared__ int tot[kWideWgCols];
    __shared__ unsigned short order[kWideWgCols], cand[kWideWgCols];
    __shared__ int nslot[kWaves];
    __shared__ unsigned long long score[kWaves], red[2][kWaves];
    __shared__ int best_s, keep_s;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * kWideWgCols;
    unsigned short* perm = wperm + (size_t)blockIdx.x * kWideWgCols;
    if (!balance || c0 + kWideWgCols > ncols) {  // uniform: the identity
        for (int i = tid; i < kWideWgCols; i += nt) {
            perm[i] = (unsigned short)i;
            if (c0 + i < ncols) winv[c0 + i] = (unsigned short)i;
        }
        return;
    }
    const int* blk = cnt + c0;  // blk[c * ncols + col]
    int* L = L0 + (size_t)blockIdx.x * kWaves * nch;
    for (int col = tid; col < kWideWgCols; col += nt) {
        int s = 0;
        for (int c = 0; c < nch; ++c) s += blk[(size_t)c * ncols + col];
        tot[col] = s;
    }
    for (int i = tid; i < kWaves * nch; i += nt) L[i] = 0;
    if (tid < kWaves) nslot[tid] = 0;
    __syncthreads();
    for (int i = tid; i < kWideWgCols; i += nt) {
        int r = 0;
        for (int j = 0; j < kWideWgCols; ++j) r += (tot[j] > tot[i] || (tot[j] == tot[i] && j < i)) ? 1 : 0;
        order[r] = (unsigned short)i;
    }
    __syncthreads();
    for (int step = 0; step < kWideWgCols; ++step) {
        const int col = order[step];
        const int* cc = blk + col;
        unsigned long long s = 0;  // wave w scores wave-column w
        if (nslot[wave] < kWideCW)
            for (int c = lane; c < nch; c += 64)
                s += (unsigned long long)L[(size_t)wave * nch + c] * (unsigned long long)cc[(size_t)c * ncols];
        s = wave_sum(s);
        if (lane == 0) score[wave] = s;
        __syncthreads();
        if (tid == 0) {
            int best = -1;
            for (int w = 0; w < kWaves; ++w)
                if (nslot[w] < kWideCW && (best < 0 || score[w] < score[best])) best = w;
            cand[best * kWideCW + nslot[best]++] = (unsigned short)col;
            best_s = best;
        }
        __syncthreads();
        const int bw = best_s;
        for (int c = tid; c < nch; c += nt) L[(size_t)bw * nch + c] += cc[(size_t)c * ncols];
        __syncthreads();
    }
    // keep the deal only where it lowers sum_c max_w L[w][c]
    unsigned long long sg = 0, si = 0;
    for (int c = tid; c < nch; c += nt) {
        int mg = 0, mi = 0;
        for (int w = 0; w < kWaves; ++w) {
            mg = max(mg, L[(size_t)w * nch + c]);
            int s = 0;
            for (int j = 0; j < kWideCW; ++j) s += blk[(size_t)c * ncols + w * kWideCW + j];
            mi = max(mi, s);
        }
        sg += (unsigned long long)mg;
        si += (unsigned long long)mi;
    }
    sg = wave_sum(sg);
    si = wave_sum(si);
    if (lane == 0) {
        red[0][wave] = sg;
        red[1][wave] = si;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long g = 0, i = 0;
        for (int w = 0; w < kWaves; ++w) {
            g += red[0][w];
            i += red[1][w];
        }
        keep_s = g < i ? 1 : 0;
    }
    __syncthreads();
    const bool keep = keep_s != 0;
    for (int i = tid; i < kWideWgCols; i += nt) {
        const int v = keep ? cand[i] : i;
        perm[i] = (unsigned short)v;
        winv[c0 + v] = (unsigned short)i;
    }
}

// The counts in slot order: cntp[c*ncols + b*352 + p] = cnt[c*ncols + b*352 +
// wperm[b*352 + p]] (p = 22 * wave + slot), so that a wave's columns are again
// one range of every chunk row and the prefix sums below serve as before.
__global__ void k_wide_permute_counts(const int* __restrict__ cnt, const unsigned short* __restrict__ wperm, int ncols,
                                      int nch, int* __restrict__ cntp) {
    const long long total = (long long)nch * ncols;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i <= total;
         i += (long long)gridDim.x * blockDim.x) {
        if (i == total) {
            cntp[i] = 0;
            continue;
        }
        const int q = (int)(i % ncols), b0 = q / kWideWgCols * kWideWgCols;
        cntp[i] = cnt[i - q + b0 + wperm[q]];
    }
}

// Per column block: sum_c max_w (entries of wave w in chunk c) and the number
// of (wave, chunk) streams longer than the generated loop's scalar buffer, for
// the contiguous assignment (st[0], st[2]) and the map in use (st[1], st[3]).
__global__ void k_wide_stats(const int* __restrict__ cnt, const unsigned short* __restrict__ wperm, int ncols, int nch,
                             unsigned long long* __restrict__ st) {
    const int c0 = blockIdx.x * kWideWgCols;
    const unsigned short* perm = wperm + (size_t)blockIdx.x * kWideWgCols;
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int c = threadIdx.x; c < nch; c += blockDim.x) {
        const int* row = cnt + (size_t)c * ncols + c0;
        int mi = 0, mp = 0;
        for (int w = 0; w < kWaves; ++w) {
            int si = 0, sp = 0;
            for (int j = 0; j < kWideCW; ++j) {
                const int ci = w * kWideCW + j, cp = perm[ci];
                si += c0 + ci < ncols ? row[ci] : 0;
                sp += c0 + cp < ncols ? row[cp] : 0;
            }
            mi = max(mi, si);
            mp = max(mp, sp);
            v[2] += si > TCSCW_GEN_CAP ? 1 : 0;
            v[3] += sp > TCSCW_GEN_CAP ? 1 : 0;
        }
        v[0] += (unsigned long long)mi;
        v[1] += (unsigned long long)mp;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(st + k, s);
    }
}

// gcnt[gw*nch + c] = header + entries of wide group gw in chunk c (group-major);
// cptr is the prefix sum of the counts in slot order, where group gw is the
// range [wide_group_col0(gw), + 22) cut at ncols (a partial block keeps the identity)
__global__ void k_wide_group_counts(const int* __restrict__ cptr, int ncols, int nch, int Gw, int* __restrict__ gcnt) {
    const long long total = (long long)nch * Gw;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(i / nch), c = (int)(i % nch);
        const int n0 = wide_group_col0(g), n1 = min(n0 + kWideCW, ncols);
        gcnt[i] = kHdr + cptr[(long long)c * ncols + n1] - cptr[(long long)c * ncols + n0];
    }
}

__global__ void k_wide_scatter(const int2* __restrict__ ent, const int* __restrict__ sptr, int G, int nch, int ncols,
                               const int* __restrict__ cptr, const unsigned short* __restrict__ winv,
                               const int* __restrict__ sptr_w, int2* __restrict__ ent_w) {
    const long long total = (long long)G * nch;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(i / nch), c = (int)(i % nch);
        int first;
        const int n = stream_range(sptr, i, &first);
        const int n0 = group_col0(g);
        int rank = 0, slot = -1, base = 0, jw = 0;
        for (int e = 0; e < n; ++e) {
            const int2 v = ent[first + e];
            if (is_pad(v.y)) continue;
            const int s = (v.y & 0x3ff) >> 2;
            if (s != slot) {  // the next column: its wide group and slot there (the slot map), its first
                slot = s;     // position = the entries of the group's lower slots in this chunk
                rank = 0;
                const int col = n0 + s;
                const int p = col / kWideWgCols * kWideWgCols + winv[col];  // the column in slot order
                const int gw = (p / kWideWgCols) * kWaves + (p % kWideWgCols) / kWideCW;
                jw = p - wide_group_col0(gw);
                base = sptr_w[(long long)gw * nch + c] + kHdr +
                       (cptr[(long long)c * ncols + p] - cptr[(long long)c * ncols + wide_group_col0(gw)]);
            }
            ent_w[base + rank++] = make_int2(v.x, (v.y & ~0x3ff) | (4 * jw));
        }
    }
}

// Chunk headers {whole batches, rest}, {bytes to the next header, 0}; after
// the last stream the empty chain of idle waves and the guard entries
// (k_fill_headers of tcsc_kernels.hip, with the wide loop's batch).
__global__ void k_wide_headers(const int* __restrict__ sptr_w, int nch, int Gw, int2* __restrict__ ent_w,
                               long long n_entries) {
    const long long total = (long long)nch * Gw;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int s0 = sptr_w[i], s1 = sptr_w[i + 1];
        const int n = s1 - s0 - kHdr;
        ent_w[s0] = make_int2(n / kWideBatch, n % kWideBatch);
        ent_w[s0 + 1] = make_int2((s1 - s0) * (int)sizeof(int2), 0);
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < kEntGuard; i += blockDim.x)
            ent_w[n_entries + i] = i < kHdr ? make_int2(0, 0) : make_int2(0x3f800000, kTK << 10);
}

inline int grid_for(long long n, int block) {
    long long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 65535LL * 16) g = 65535LL * 16;
    return (int)g;
}

}  // namespace

// Phase 1: cnt (zeroed here, per column) -> the slot map (wperm, its inverse
// winv, the statistics wstats[4] of k_wide_stats) -> cptr (nch*ncols + 1: the
// counts in slot order, summed in place), gcnt (Gw*nch + 1, the last 0) ->
// sptr_w.  tmp serves exclusive scans of either length.
hipError_t wide_counts(const int2* ent, const int* sptr, int G, int nch, int ncols, int Gw, int balance, int* cnt,
                       int* cptr, int* gcnt, int* sptr_w, int* loads, unsigned short* wperm, unsigned short* winv,
                       unsigned long long* wstats, void* tmp, size_t tmp_bytes, hipStream_t st) {
    hipError_t e;
    const long long nc = (long long)nch * ncols, ng = (long long)nch * Gw;
    const int nblk = wide_blocks_for(ncols);
    if ((e = hipMemsetAsync(cnt, 0, (size_t)(nc + 1) * sizeof(int), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(gcnt + ng, 0, sizeof(int), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(wstats, 0, 4 * sizeof(unsigned long long), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_wide_col_counts, dim3(grid_for((long long)G * nch, 128)), dim3(128), 0, st, ent, sptr, G, nch,
                       ncols, cnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_wide_balance, dim3(nblk), dim3(kWaves * 64), 0, st, cnt, ncols, nch, balance, loads, wperm,
                       winv);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_wide_stats, dim3(nblk), dim3(256), 0, st, cnt, wperm, ncols, nch, wstats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_wide_permute_counts, dim3(grid_for(nc + 1, 256)), dim3(256), 0, st, cnt, wperm, ncols, nch,
                       cptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = tmp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, cptr, cptr, (int)(nc + 1), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_wide_group_counts, dim3(grid_for(ng, 256)), dim3(256), 0, st, cptr, ncols, nch, Gw, gcnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tb = tmp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(tmp, tb, gcnt, sptr_w, (int)(ng + 1), st);
}

// Phase 2: ent_w (n_entries + kEntGuard entries) from the 16-column streams.
hipError_t wide_fill(const int2* ent, const int* sptr, int G, int nch, int ncols, int Gw, const int* cptr,
                     const unsigned short* winv, const int* sptr_w, int2* ent_w, long long n_entries, hipStream_t st) {
    hipLaunchKernelGGL(k_wide_scatter, dim3(grid_for((long long)G * nch, 128)), dim3(128), 0, st, ent, sptr, G, nch,
                       ncols, cptr, winv, sptr_w, ent_w);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_wide_headers, dim3(grid_for((long long)nch * Gw, 256)), dim3(256), 0, st, sptr_w, nch, Gw,
                       ent_w, n_entries);
    return hipGetLastError();
}

// The gather launch of launch_gemm for GemmArgs::geo == kWideCW: g.ent, g.sptr,
// g.n_entries and g.n_groups are the wide streams; X^T is staged already.
hipError_t launch_stream_wide(const GemmArgs& g, hipStream_t st) {
    if (g.order != 0 || g.ent == nullptr || g.wperm == nullptr) return hipErrorInvalidValue;
    const int nch = (g.K + kTK - 1) / kTK;
    const int ldxt = ldxt_for(g.M);
    dim3 grid((g.n_groups + kWaves - 1) / kWaves, (g.M + kTM - 1) / kTM, 1);
    dim3 block(kWaves * 64);
    int pfd = 0, pfl = 1;
    pf_stream_params(g.n_entries, g.n_groups, nch, &pfd, &pfl);
#define TCSC_LAUNCH_W(BF, PR)                                                                                \
    hipLaunchKernelGGL((k_stream_w<BF, PR>), grid, block, 0, st, g.XT, g.ent, g.sptr, g.B, g.Y, g.wperm, g.n_entries, \
                       ldxt, g.M, g.n_groups, g.ncols, nch, g.ldy, g.a, pfd, pfl)
    if (g.bias_first) {
        if (g.prelu) TCSC_LAUNCH_W(true, true);
        else TCSC_LAUNCH_W(true, false);
    } else {
        if (g.prelu) TCSC_LAUNCH_W(false, true);
        else TCSC_LAUNCH_W(false, false);
    }
#undef TCSC_LAUNCH_W
    return hipGetLastError();
}

}  // namespace tcsc
