/*
 * tcsc_gpu.h -- device-pointer extension of the TCSC drop-in API.
 *
 * The reference's API (sparse/tcsc.h:19-48) only takes host pointers and is
 * synchronous, so a call through it always pays PCIe transfers.  These entry
 * points expose the same computation on device-resident buffers, on a caller
 * supplied HIP stream, so that kernel-only throughput can be measured and so
 * that one process per GPU (torch.distributed ranks, MPI ranks, ...) can run
 * its own column shard.  Plain C ABI: no HIP or torch types in the
 * signatures; streams are passed as `void*` (a hipStream_t, NULL = the
 * device's null stream).
 *
 * A plan is the device-side image of (a column range of) one tcsc_t,
 * re-laid out for the gfx950 gather kernel ("Data layout in
 * HBM").  Building a plan is the only place W's index arrays cross PCIe.
 */
#ifndef TCSC_AMD_TCSC_GPU_H
#define TCSC_AMD_TCSC_GPU_H

#include <stddef.h>
#include "sparse/tcsc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which reference entry point a launch stands in for.  The GPU computes all
 * of them with one kernel family; the variant only selects the epilogue
 * (PReLU or not).  See DESIGN.md "Numerics" for the summation order. */
enum tcsc_variant {
    TCSC_VARIANT_BASIC = 0,            /* tcsc_sgemm_basic                    tcsc.c:69  */
    TCSC_VARIANT_OPTIMIZED = 1,        /* tcsc_sgemm_optimized                tcsc.c:101 */
    TCSC_VARIANT_PRELU_BASIC = 2,      /* tcsc_sgemm_prelu_basic              tcsc.c:143 */
    TCSC_VARIANT_PRELU_SEPARATE = 3,   /* tcsc_sgemm_prelu_optimized_separate tcsc.c:179 */
    TCSC_VARIANT_PRELU_ONTHEGO = 4,    /* tcsc_sgemm_prelu_optimized_onthego  tcsc.c:231 */
    TCSC_VARIANT_SPARSE_GEMM = 5       /* sparseGEMM<float>          SparseGEMM.h:104-119:
                                          y = 0 + sum(+1 rows) - sum(-1 rows); Y = y + b.
                                          sparseGEMM_PReLU<float> (SparseGEMM.h:151-168)
                                          is TCSC_VARIANT_PRELU_BASIC: the same order
                                          as tcsc.c:143-165, the same predicate     */
};

/* Status codes (0 = success).  HIP errors are passed through as
 * TCSC_E_HIP; the message is in tcsc_gpu_last_error(). */
enum tcsc_status {
    TCSC_OK = 0,
    TCSC_E_ARG = 1,      /* bad argument (shape mismatch, NULL, range)   */
    TCSC_E_HIP = 2,      /* a HIP runtime call failed                     */
    TCSC_E_NOMEM = 3,    /* host or device allocation failed              */
    TCSC_E_NODEV = 4     /* no usable gfx950 device                       */
};

/* Summation order of the gather.  FAST (default): each output column adds
 * its +1 and -1 rows merged in ascending k; the five variants then agree with
 * the reference within the fp32 bound of DESIGN.md "Numerics" and bit for bit
 * on integer-valued inputs.  REFERENCE: the order of each reference variant
 * (tcsc.c:84-93 for basic, :149-161 prelu_basic, :113-137 the optimized
 * family), so float outputs are bit-identical to the reference compiled with
 * IEEE semantics, at about twice the kernel time (K is walked once per
 * sign).  Chosen per plan at creation time (tcsc_gpu_set_order, or
 * TCSC_ORDER=reference in the environment). */
enum tcsc_order {
    TCSC_ORDER_FAST = 0,
    TCSC_ORDER_REFERENCE = 1
};

typedef struct tcsc_gpu_plan tcsc_gpu_plan;

typedef struct {
    int device;          /* HIP device ordinal the plan lives on          */
    int rows;            /* K                                             */
    int cols;            /* columns in this plan (col_end - col_begin)    */
    int col_begin;       /* first column of W covered                     */
    long long nnz;       /* +1 and -1 entries in the covered columns      */
    long long n_pos, n_neg;
    int chunk_k;         /* K rows per LDS chunk used by the kernel       */
    int n_chunks;        /* ceil(K / chunk_k)                             */
    size_t device_bytes; /* HBM held by the plan                          */
    int order;           /* enum tcsc_order the plan was built for        */
    int mfma_min_M;      /* > 0: the plan holds the MFMA image of W (denser
                            W, see tcsc_gpu_sgemm) and launches with
                            M >= mfma_min_M may use it (the cost model;
                            tcsc_gpu_launch_info says which path a given
                            M takes); 0: gather only                      */
} tcsc_gpu_plan_info;

/* Number of HIP devices visible (0 when there is no GPU). */
int tcsc_gpu_device_count(void);

/* Summation order for plans created from now on, including the plans the
 * host-pointer API (sparse/tcsc.h) builds for its cache (a cached tcsc_t is
 * rebuilt when the order changes).  Process-wide; default from $TCSC_ORDER. */
void tcsc_gpu_set_order(int order);
int tcsc_gpu_get_order(void);

/* Upload columns [col_begin, col_end) of W to `device` and build the plan.
 * W is read on the host; `stream` orders the uploads and the build kernels.
 * The call returns after the plan is complete (it synchronises `stream`). */
int tcsc_gpu_plan_create(const tcsc_t *W, int col_begin, int col_end,
                         int device, void *stream, tcsc_gpu_plan **out);

/* Same, from raw TCSC arrays that already live on `device` (the layout of
 * tcsc_t: col_start_* have cols+1 entries, absolute offsets).  Nothing
 * crosses PCIe. */
int tcsc_gpu_plan_create_device(int rows, int cols,
                                const int *d_col_start_pos,
                                const int *d_col_start_neg,
                                const int *d_row_index_pos,
                                const int *d_row_index_neg,
                                int col_begin, int col_end, int device,
                                void *stream, tcsc_gpu_plan **out);

int tcsc_gpu_plan_get_info(const tcsc_gpu_plan *plan, tcsc_gpu_plan_info *info);

/* Which kernels a tcsc_gpu_sgemm of M rows on this plan runs (with X 16-B
 * aligned, the plan's reserved workspace and the current environment):
 *   TCSC_PATH_GATHER k_transpose + k_stream (+ k_reduce, or the in-launch
 *                    combine: tcsc_gpu_launch_combine)
 *   TCSC_PATH_MFMA   k_split3 + k_gemm3 + k_fixup, or with K split
 *                    k_split3 + k_gemm3 + k_reduce_fix (the slabs and the
 *                    fixup in one kernel), denser W (the cost model)
 *   TCSC_PATH_SMALL  k_small_m, M <= 4 (X and -X fit the LDS)
 * and *slices = the K split (1 = none): the gather's, or the MFMA GEMM's on
 * grids of few 128 x 128 tiles (M <= 256 at N = 8192: partial sums of whole
 * 64-k blocks, added in slice order). */
enum tcsc_path {
    TCSC_PATH_GATHER = 0,
    TCSC_PATH_FUSED = 1, /* retired (round 5): the persistent k_fused left the library; never returned */
    TCSC_PATH_MFMA = 2,
    TCSC_PATH_SMALL = 3,
    TCSC_PATH_DECODE = 4 /* k_decode8: int8 calls of M <= 16 rows (k_decode8r: up to 64 where the plan's
                            tcsc_gpu_plan_set_decode_rows setting admits them) on a plan with the 2-bit image
                            (tcsc_gpu_plan_enable_w2); never an fp32 or bf16 call */
};
int tcsc_gpu_launch_info(const tcsc_gpu_plan *plan, int M, int *path, int *slices);

/* For TCSC_PATH_GATHER with a K split, where the split-K slabs are combined
 * (N % 4 == 0 and the plan's reserved workspace needed for either in-launch
 * form; TCSC_COMBINE=0 turns both off, =1 lifts the band form's size rule):
 *   4  inside the k_stream launch, pairwise in split halves (exactly 2
 *      slices, the grid fits the chip at one workgroup per CU: each slice
 *      stores half its partial and finalizes the other half)
 *   3  inside the k_stream launch, pairwise (exactly 2 slices: the tile's
 *      first slice to finish stores its slab, the second combines; any grid)
 *   2  inside the k_stream launch, by row bands (>= 3 slices, the grid fits
 *      the chip at one workgroup per CU, >= 64 workgroups)
 *   0  by k_reduce after it, or nothing is split.
 * A Y or bias that is not 16-B aligned, or an ldy that is no multiple of 4,
 * makes the launch fall back to k_reduce after k_stream; the query has no
 * pointers to look at and reports the aligned case. */
int tcsc_gpu_launch_combine(const tcsc_gpu_plan *plan, int M, int *in_launch);

/* The gather kernel's geometry a tcsc_gpu_sgemm of M rows takes:
 * *cols_per_wave = 16 (k_stream: 256 columns per workgroup), 22 (k_stream_w:
 * 352 columns per workgroup; unsplit K, the fast order, a plan whose
 * tcsc_gpu_plan_reserve built the second copy of the entry streams) or 0 when
 * the launch is not on TCSC_PATH_GATHER.  The two compute the same bits; the
 * choice is a rounds model, tcsc_gpu_wide_pays, unless TCSC_GEO=16|22 forces
 * one (22 is an error where K is split by TCSC_SLICES, the order is the
 * reference's or the plan has no wide streams). */
int tcsc_gpu_launch_geometry(const tcsc_gpu_plan *plan, int M, int *cols_per_wave);
/* The rounds model itself (pure; no device needed): 1 when M rows x ncols
 * columns on num_cus CUs take fewer column-rounds with 352-column workgroups
 * than with 256-column ones, weighted by the measured cost per column. */
int tcsc_gpu_wide_pays(int M, int ncols, int num_cus);
/* The slot map of a plan's 22-column streams and what it buys (read-only; an
 * error on a plan without them).  A workgroup of k_stream_w covers a block of
 * 352 columns with 16 waves of 22 slots; slot j of wave w of block b owns the
 * block's column map[b * 352 + w * 22 + j].  tcsc_gpu_plan_reserve deals every
 * full block's columns to its waves so that the busiest wave of each 48-row
 * chunk of K, for which the other 15 wait, has fewer entries; the last, partial
 * block, and every block of a plan reserved under TCSC_WIDE_BALANCE=0, keep
 * the identity (wave w owns columns 22 w .. 22 w + 21).  Outputs are the same
 * bits under any map.  With L[w][c] = the nonzeros of wave w's columns in
 * chunk c:
 *   stats[0], stats[1]  sum over blocks and chunks of max_w L[w][c], for the
 *                       identity and for the map in use
 *   stats[2], stats[3]  the (wave, chunk) streams with L[w][c] > 30, the
 *                       kernel's scalar entry buffer, for either
 * map (may be NULL, like stats) receives the map: map_entries must be
 * 352 * ceil(cols / 352).  Copies from the device and synchronises. */
int tcsc_gpu_plan_wide_stats(const tcsc_gpu_plan *plan, long long stats[4], unsigned short *map,
                             size_t map_entries);

/* Allocate the plan's workspace for launches of up to `max_M` rows: X^T
 * (K x max_M rounded up to 256 floats; the kernel streams X^T rows into LDS)
 * plus, where the gather's cost model or the MFMA GEMM's grid splits K over
 * workgroups, the fp32 partial slabs combined in a fixed order.  Both split K
 * more at smaller M, so the slabs can peak below max_M: the workspace is sized
 * for the largest need of every M <= max_M on every path the plan has (with
 * the $TCSC_SLICES / $TCSC_MFMA_WGS / $TCSC_SMALL_M in force at this call).
 * Optional: tcsc_gpu_sgemm grows the workspace itself on the first call that
 * needs more (that call then allocates and synchronises the device, and a
 * graph captured before it holds the freed workspace); reserving up front
 * keeps every sgemm call of every M <= max_M allocation-free.  Not
 * thread-safe against concurrent launches of the same plan. */
int tcsc_gpu_plan_reserve(tcsc_gpu_plan *plan, int max_M);
void tcsc_gpu_plan_destroy(tcsc_gpu_plan *plan);

/* Workspace arithmetic of a plan, on the host (no launch, no allocation):
 * *need = the workspace bytes a tcsc_gpu_sgemm of M rows wants on `path`,
 * *reserved = the bytes the plan holds now.  `path` is TCSC_PATH_AUTO (the
 * path tcsc_gpu_launch_info names for this M) or one of TCSC_PATH_GATHER,
 * TCSC_PATH_MFMA, TCSC_PATH_SMALL: what that path would need at this M
 * whatever the cost model prefers, 0 where the plan cannot run it (no MFMA
 * image, M below mfma_min_M, M > 4 or an X too long for the small-M path).
 * TCSC_PATH_DECODE may be named too: k_decode8 needs no workspace, so its need
 * is 0 at every M.
 * The gather's need is its X^T plus the split-K slabs of the split the cost
 * model (or $TCSC_SLICES) picks with room to spare.  After
 * tcsc_gpu_plan_reserve(max_M), need <= reserved for every M <= max_M and
 * every path.  Either output pointer may be NULL. */
#define TCSC_PATH_AUTO (-1)
int tcsc_gpu_plan_workspace(const tcsc_gpu_plan *plan, int M, int path, size_t *need, size_t *reserved);

/* Y[m, j] = act(B[j] + sum_{k in P(j)} X[m,k] - sum_{k in Q(j)} X[m,k])
 * for m < M and the plan's columns j < cols.
 *   dX : M x K row-major device array (K = plan rows), 4-byte aligned
 *   dB : `cols` floats (the plan's slice of the bias)
 *   dY : M rows with pitch `ldy` floats (ldy >= cols); columns beyond
 *        `cols` are not touched
 *   act: PReLU(v) = (v < 0 ? a*v : v) for the PRELU variants, identity
 *        otherwise.
 *   M  : any; the gather path runs more than 2^22 rows as several
 *        launches (offsets are 64-bit, so M*K may exceed 2^31).
 * Asynchronous on `stream`; once the workspace covers M (see
 * tcsc_gpu_plan_reserve) no allocation and no synchronisation (safe to
 * capture in a hipGraph).
 * Denser W (density >= 0.055, see tcsc_gpu_plan_info.mfma_min_M): launches
 * with M >= mfma_min_M run the MFMA path where a per-launch cost model says
 * it beats the gather (measured crossover ~0.08 at M >= 2048, ~0.04-0.1 at
 * M <= 256 for K = N = 8192, lower for smaller K and N) -- X
 * split exactly into three bf16 parts (k_split3) and one bf16 GEMM with fp32
 * accumulation against the plan's bf16 image of W on the matrix cores
 * (k_gemm3, the library's own gfx950 kernel, bias and PReLU fused in its
 * store; a grid with fewer tiles than the chip runs at once splits K into
 * slices of whole 64-k blocks whose partial sums k_reduce_fix adds in slice
 * order with the bias and PReLU), then the exact fixup of
 * rows holding non-finite or tiny values (k_fixup) -- with the same accuracy
 * bounds as the gather.  It allocates nothing per launch and
 * keeps no state between launches, so graph replays with new X are exact.
 * $TCSC_PATH=gather|mfma at plan creation disables / forces the path (the
 * image is never built for K of ~2.8 M rows or more: k_gemm3's staging
 * offsets are 32-bit; the gather serves those plans).
 * Thread safety: concurrent launches of ONE plan (on any streams) share its
 * workspace and are not supported; different plans are independent. */
int tcsc_gpu_sgemm(const tcsc_gpu_plan *plan, const float *dX, const float *dB,
                   float *dY, int M, int ldy, int variant, float a,
                   void *stream);

/* The two halves of tcsc_gpu_sgemm, for callers that time them apart or
 * reuse one staging of X for several launches of the same plan:
 * tcsc_gpu_prepare_x writes X (M x K) transposed into the plan's workspace
 * (kernel k_transpose); tcsc_gpu_sgemm_prepared then runs the gather
 * (k_stream, plus k_reduce when K is split) on that staged X for the same
 * M.  Same stream semantics as tcsc_gpu_sgemm. */
int tcsc_gpu_prepare_x(const tcsc_gpu_plan *plan, const float *dX, int M, void *stream);
int tcsc_gpu_sgemm_prepared(const tcsc_gpu_plan *plan, const float *dB, float *dY, int M, int ldy,
                            int variant, float a, void *stream);

/* tcsc_gpu_sgemm for bf16 activations: the same Y (fp32) from X given as
 * bf16, with no fp32 copy of X made by the caller.
 *   dX_bf16 : M x K row-major, contiguous array of bf16 bit patterns
 *             (uint16_t, the high half of the fp32 value), 2-byte aligned
 *   dB, dY, ldy, variant, a, stream : exactly as in tcsc_gpu_sgemm
 * Every bf16 value is an fp32 value and W is exact in bf16, so the numeric
 * contract is tcsc_gpu_sgemm's on the widened X: bit-exact on integer-valued
 * inputs, within 2^-20 (|b| + sum |x|) otherwise; on one path and K split the
 * bits are those of tcsc_gpu_sgemm(X widened to fp32).
 *   gather : k_transpose's bf16 form widens X into the same fp32 X^T; k_stream, the
 *            reduce and the in-launch combine are the fp32 call's
 *   small  : k_small_m stages the widened rows (M <= 4)
 *   MFMA   : k_pack1 (X -> X1, M x 64-k blocks of bf16, and the row flags
 *            by k_split3's rule: a non-finite x or a nonzero |x| < 2^-100),
 *            the one-part k_gemm3 -- one sub-step per 64-k block instead of
 *            three -- and the one-part k_fixup / k_reduce_fix
 * Same guarantees: asynchronous on `stream`, allocation-free once the
 * workspace covers M, capturable in a graph, M > 2^22 rows on the gather as
 * several launches; the same argument checks, answered with TCSC_E_ARG before
 * any HIP call.  Works on every plan (forward, transposed, reference order --
 * gather only, as for fp32 -- and column shards).
 * Workspace: for every M and path no more than tcsc_gpu_plan_workspace reports
 * for the fp32 call (the gather's is the same; the MFMA path's holds X1, a
 * third of X3; the small-M path needs none), so tcsc_gpu_plan_reserve(max_M)
 * covers bf16 launches as it is.
 * Routing: the fp32 call's cost model with the GEMM term and the K walk
 * divided by 3; $TCSC_PATH, $TCSC_SLICES, $TCSC_MFMA_WGS and
 * $TCSC_SMALL_M act as on the fp32 call.  tcsc_gpu_launch_info_bf16 reports
 * what a bf16 call of M rows runs (as tcsc_gpu_launch_info does for fp32).
 * Out of scope: a host-pointer version, bf16 Y (the int8 call has one on its
 * decode and MFMA routes: tcsc_gpu_sgemm_i8_out), bf16 B, and a
 * prepare_x / sgemm_prepared pair for bf16. */
int tcsc_gpu_sgemm_bf16(const tcsc_gpu_plan *plan, const void *dX_bf16, const float *dB,
                        float *dY, int M, int ldy, int variant, float a, void *stream);
int tcsc_gpu_launch_info_bf16(const tcsc_gpu_plan *plan, int M, int *path, int *slices);

/* ---- int8 activations with a per-row scale -------------------
 * What ternary-weight models (BitNet b1.58 and relatives) run: X quantized to
 * int8 per token, W about two thirds nonzero, so the MFMA path.
 *
 * tcsc_gpu_plan_enable_i8: on a plan that holds the bf16 MFMA image, build an
 * int8 image of W^T beside it (cols rows of K rounded up to 128 bytes, made on
 * the device from the bf16 image; counted in device_bytes, freed with the
 * plan).  It is built only if every |w| <= 127 and every column's sum of |w|
 * is below 2^24, which keeps |sum_k q w| below 2^31 for any int8 X.  Otherwise,
 * and on a gather-only or reference-order plan, the call returns TCSC_OK and
 * leaves the plan as it was (tcsc_gpu_plan_has_i8 then says 0, and int8 calls
 * run the gather or the small-M path).  Idempotent; synchronises `stream`.
 * Nothing else in the library allocates the image: a plan that never calls
 * this behaves exactly as before.
 *
 * tcsc_gpu_sgemm_i8:  Y[m, j] = act(s[m] * sum_k q[m, k] W[k, j] + b[j])
 *   dXq    : M x K row-major, contiguous int8 (any alignment, every value
 *            -128 .. 127)
 *   dScale : M floats s[m], or NULL for all ones
 *   dB, dY, ldy, variant, a, stream : exactly as in tcsc_gpu_sgemm
 * The bf16 call's guarantees: asynchronous on `stream`, allocation-free once
 * the workspace covers M (tcsc_gpu_plan_reserve covers int8 launches as it is:
 * X8 is a sixth of X3, there are no flags, the i32 slabs never outnumber the
 * fp32 ones), capturable, the same argument checks answered with TCSC_E_ARG
 * before any HIP call; forward, transposed, reference-order and column-shard
 * plans; M > 2^22 rows on the gather as several launches.
 * Numerics, per path:
 *   MFMA   (the plan has the int8 image and the router picks it):
 *          Y = act(fl(fl(float(S) * s[m]) + b[j])), S the exact i32 sum,
 *          float(S) rounded to nearest, ties to even (it rounds where |S| >
 *          2^24: an odd sum below 2^25 goes to the neighbour whose mantissa
 *          is even), one multiply, one add (never fused with it), then
 *          v < 0 ? a * v : v (a NaN and -0 pass).  The same bits for every variant
 *          and every K split.  Kernels: k_pack8 (X -> X8, zero padded),
 *          k_gemm8 (v_mfma_i32_16x16x64_i8, 128-k sub-steps; the epilogue in
 *          its store), with K split raw i32 slabs and k_reduce_i8.  No row
 *          flags and no fixup: integers are never non-finite or tiny.
 *   gather and small M: the bits of tcsc_gpu_sgemm on the fp32 matrix
 *          Xs[m, k] = fl(s[m] * float(q[m, k])) on the same path and K split;
 *          the scale is folded in while staging (the int8 forms of k_transpose
 *          and of k_small_m's staging), everything after is the fp32 call's.
 *   On every path the result is exact when s is NULL or a power of two and
 *   |S| < 2^24; otherwise within 2^-20 (|b| + s sum |q|).
 * Routing: the bf16 cost model with the GEMM at twice the rate and half the
 * sub-steps per k; $TCSC_PATH, $TCSC_SLICES, $TCSC_MFMA_WGS and $TCSC_SMALL_M
 * act as on the other calls; without the int8 image the router never names
 * TCSC_PATH_MFMA.  tcsc_gpu_launch_info_i8 reports what an int8 call runs.
 *
 * tcsc_gpu_quantize_rows_i8 (k_quant_rows_i8): per row of the M x K fp32 dX,
 *   amax = max_k |x|, dScale[m] = amax / 127.0f, inv = 127.0f / amax,
 *   q = clamp(rintf(x * inv), -127, 127)   (amax = 0: q = 0, scale = 0)
 * every step one rounded fp32 operation, so a host restatement gives the same
 * bits.  A row whose maximum is so small that fl(127.0f / amax) is +inf --
 * amax <= 127 * 2^-128 = 0x02FE0000, about 3.73e-37, and every subnormal
 * maximum -- counts as a row of zeros: q = 0, scale = 0 (x * inf would be NaN
 * for x = 0 and +-127 for everything else); the loss is at most K * 3.8e-37
 * per output.  In one line: zero = !(amax > 0) || isinf(127.0f / amax).
 * Inputs must be finite (a non-finite x gives unspecified values in its own
 * row -- Xq, scale and that row of Y -- and touches no other row; never
 * a fault).  Allocates nothing, asynchronous on `stream`, capturable.
 *
 * tcsc_gpu_workspace_bound_i8 (host arithmetic, no plan, no device): the MFMA
 * workspace of an int8 and of an fp32 launch of an M x K x N problem; the
 * first never exceeds the second.
 *
 * Out of scope: int8 Y, a host-pointer version, a backward pass for the int8
 * call, and keeping X^T narrow inside the gather's LDS ring.  (A bf16 Y and
 * per-column weight scales: tcsc_gpu_sgemm_i8_out, below -- on the decode and
 * MFMA routes; on the gather and small-M routes they stay out of scope.) */
int tcsc_gpu_plan_enable_i8(tcsc_gpu_plan *plan, void *stream);
int tcsc_gpu_plan_has_i8(const tcsc_gpu_plan *plan);
int tcsc_gpu_sgemm_i8(const tcsc_gpu_plan *plan, const void *dXq, const float *dScale,
                      const float *dB, float *dY, int M, int ldy, int variant, float a, void *stream);
int tcsc_gpu_launch_info_i8(const tcsc_gpu_plan *plan, int M, int *path, int *slices);
int tcsc_gpu_quantize_rows_i8(const float *dX, int M, int K, void *dXq, float *dScale, void *stream);
int tcsc_gpu_workspace_bound_i8(int M, int K, int N, size_t *i8_bytes, size_t *f32_bytes);

/* ---- int8 decode: M <= 16 rows on a 2-bit image of W ----------
 * Token generation of a ternary-weight model is an int8 call of one row, or of
 * a batch of a few.  At M <= 16 the whole product is one 16-row MFMA tile per
 * 16 columns and the call is a stream of W, so what counts is the bytes of W
 * read: the merged CSC copy holds 4 bytes per nonzero (k_small_m, M <= 4), the
 * int8 image 1 byte per weight (k_gemm8), a ternary weight needs 2 bits.
 *
 * tcsc_gpu_plan_enable_w2: on a plan that holds the int8 image
 * (tcsc_gpu_plan_has_i8), build a 2-bit image of W beside it, on the device
 * from the int8 one (k_w2_from); counted in device_bytes, freed with the plan
 * and with the int8 image.  It is built only if every weight is -1, 0 or +1
 * (duplicate indices in W can make |w| = 2) and K < 2^22, which keeps every
 * i32 sum of the kernel below 2^31 for any int8 X.  Otherwise, and on a plan
 * without the int8 image, the call returns TCSC_OK and leaves the plan as it
 * was: tcsc_gpu_plan_has_w2 says 0 and every call behaves as before.
 * Idempotent; synchronises `stream`.  Nothing else in the library builds the
 * image: a plan that never calls this routes and computes exactly as before.
 *
 * Layout of the image: tiles of 16 columns x 256 k, 1 KiB each, column-tile
 * major then k-block, tcsc_gpu_w2_image_bytes = ceil(N/16) ceil(K/256) 1024
 * bytes in all (host arithmetic: no plan, no device).  One wave reads a tile as
 * 64 lanes x 16 contiguous bytes; lane l owns column 16 t + (l & 15) and the k
 * quarter l >> 4; dword i of its 16 bytes holds the 16 weights
 * k = 256 kb + 64 i + 16 (l >> 4) + j, j = 0 .. 15 -- the bytes of the lane's
 * v_mfma_i32_16x16x64_i8 fragment in step i of the block.  The code of weight
 * j is c = w + 1 at bit 8 (j & 3) + 2 (j >> 2), so the int8 fragment's dword d
 * is (p >> 2d) & 0x03030303.  Padding (k >= K, column >= N) holds c = 1.
 *
 * The call: tcsc_gpu_sgemm_i8 as it is.  Where the route is TCSC_PATH_DECODE,
 * k_decode8 computes
 *   Y[m, j] = act(fl(fl(float(S) * s[m]) + b[j])),   m < M <= 16, j < cols
 * with S the exact i32 sum: sum_k q c by MFMA minus the row sums sum_k q (one
 * more MFMA per step against a fragment of ones), as integers.  The epilogue is
 * the int8 MFMA path's own function, so the bits are k_gemm8's for every
 * variant and every scale, and do not depend on how K is split over the waves.
 * One launch: X is read in place (16-B loads where dXq is 16-B aligned and
 * K % 16 == 0, guarded byte loads otherwise; rows >= M are never read), the
 * waves of a workgroup split K and add their partial sums through the LDS.  No
 * workspace (tcsc_gpu_plan_workspace reports 0 for this path), no atomics, no
 * allocation, no synchronisation: capturable.  Only rows < M and columns < cols
 * are stored, with pitch ldy.
 *
 * Routing: only int8 calls on a plan with the 2-bit image take the path, and
 * only at 1 <= M <= 16 unless the plan's decode_rows setting (below, "int8
 * decode up to 64 rows") admits more.  By default it is taken where tcsc_gpu_decode_pays
 * (host arithmetic) says 1:
 *   1 <= M <= 16 and (M > 4, or the small-M path does not fit this (M, K), or
 *   16 nnz > K N)
 * -- the last clause compares the 4 bytes per nonzero of the merged CSC copy
 * with a quarter byte per weight.  $TCSC_DECODE, read per call: 0 never takes
 * the path, 1 takes it at every M <= 16 where the image exists, unset follows
 * the rule.  Where it applies it precedes the MFMA path and the small-M path.
 * tcsc_gpu_launch_info_i8 names the path; tcsc_gpu_launch_info and _bf16 never
 * do.
 *
 * Out of scope: int8 Y; a host-pointer version.  (M > 16 on the image,
 * plans that hold nothing else, and the image without the int8 one: packed
 * plans, below; M up to 64 on the decode path itself: the decode_rows setting,
 * below.) */
int tcsc_gpu_plan_enable_w2(tcsc_gpu_plan *plan, void *stream);
int tcsc_gpu_plan_has_w2(const tcsc_gpu_plan *plan);
int tcsc_gpu_w2_image_bytes(int K, int N, size_t *bytes);
int tcsc_gpu_decode_pays(int M, int K, int N, long long nnz);

/* ---- packed plans: int8 calls at every M from the 2-bit image alone
 * A plan that decodes as above still holds every format of W: the gather's
 * entry streams (about 8 bytes per nonzero), the merged CSC copy (4 per
 * nonzero), the bf16 image (2 per weight), the int8 image (1) and the 2-bit
 * image (1/4).  A packed plan holds the last one and nothing else of W.
 *
 * tcsc_gpu_plan_create_packed / _packed_device: the arguments of
 * tcsc_gpu_plan_create / _create_device.  The image is built on the device
 * straight from the TCSC arrays (k_w2_from_tcsc; integer adds only, so no
 * order of execution shows in it) and is byte for byte the one
 * tcsc_gpu_plan_enable_i8 + _enable_w2 build for the same W and column range:
 * the layout above, padding code 1, a +1 and a -1 at one position cancel, and
 * the order inside a column does not matter.  Straight after creation
 * tcsc_gpu_plan_get_info(...).device_bytes == tcsc_gpu_w2_image_bytes(K, cols)
 * exactly; nnz, n_pos, n_neg, rows, cols and col_begin are filled, mfma_min_M
 * is 17, chunk_k is the library's constant and n_chunks is 0.  TCSC_E_ARG with
 * a message, and no plan, for: a position whose summed weight is outside
 * {-1, 0, +1} (a duplicated index), K < 1 or K >= 2^22, a col_start that is no
 * range or a row outside [0, K), and a reference-order request
 * ($TCSC_ORDER=reference or tcsc_gpu_set_order) -- a packed plan has no other
 * format to fall back to.  $TCSC_PATH is not read.  Synchronises `stream`.
 *
 * tcsc_gpu_sgemm_i8 on a packed plan (the numeric contract of the int8 MFMA
 * path, Y = act(fl(fl(float(S) * s[m]) + b[j])) with S the exact i32 sum: the
 * bits of k_gemm8 on an ordinary plan of the same W, for every variant, K
 * split and tile shape):
 *   1 <= M <= 16  TCSC_PATH_DECODE, k_decode8 as it is -- whatever
 *                 tcsc_gpu_decode_pays or $TCSC_DECODE say: there is nothing
 *                 else to run
 *   17 <= M <= 64 TCSC_PATH_DECODE too, k_decode8r, where the plan's decode_rows
 *                 setting admits M (tcsc_gpu_plan_set_decode_rows; by default
 *                 it admits none and the next line holds from 17 rows)
 *   M >= 17       TCSC_PATH_MFMA: k_pack8 (X -> X8), then k_gemm8w2, k_gemm8
 *                 with the B fragments loaded from the 2-bit image straight
 *                 into registers and turned into signed bytes there (no row
 *                 sums), on k_gemm8's tiles and K split (mfma8_slices;
 *                 $TCSC_MFMA_WGS acts as on other plans), with K split raw i32
 *                 slabs and k_reduce_i8
 *   M > 2^22      several launches of at most 2^22 rows on one workspace
 * tcsc_gpu_launch_info_i8 reports this; tcsc_gpu_plan_reserve and
 * tcsc_gpu_plan_workspace size X8 and the slabs for every M <= max_M (0 for the
 * decode path), after which calls allocate nothing and can be captured.
 * $TCSC_PATH=gather has nothing to select and is ignored.
 * Everything that needs a format the plan lacks returns TCSC_E_ARG with a
 * message naming the call and "packed plan", before any HIP call:
 * tcsc_gpu_sgemm, _sgemm_bf16, _prepare_x, _sgemm_prepared, _sgemm_t,
 * tcsc_gpu_launch_info, _launch_info_bf16, _launch_geometry and
 * _launch_combine.  tcsc_gpu_plan_enable_i8 and _enable_w2 return TCSC_OK and
 * change nothing; tcsc_gpu_plan_has_w2 says 1 and tcsc_gpu_plan_has_i8 0.
 *
 * tcsc_gpu_plan_copy_w2: a device-to-device copy of the image of any plan that
 * has one (packed or after tcsc_gpu_plan_enable_w2) into d_dst, asynchronous
 * on `stream`; TCSC_E_ARG if the plan has no image or `bytes` is not
 * tcsc_gpu_w2_image_bytes(K, cols).  The first half of saving a packed model.
 *
 * On an ordinary plan that has the 2-bit image, $TCSC_W2GEMM=1 (read per call)
 * sends the int8 calls that route to TCSC_PATH_MFMA through k_gemm8w2 instead
 * of k_gemm8: the same route, slices, workspace and bits (the A/B on one plan;
 * unset or 0 changes nothing, and it is never a default).
 *
 * Out of scope: fp32 or bf16 activations, a backward pass, packed transposed
 * plans, a host-pointer version, int8 Y.  (Loading a packed plan from a
 * saved image: the block after this one.) */
int tcsc_gpu_plan_create_packed(const tcsc_t *W, int col_begin, int col_end,
                                int device, void *stream, tcsc_gpu_plan **out);
int tcsc_gpu_plan_create_packed_device(int rows, int cols,
                                       const int *d_col_start_pos,
                                       const int *d_col_start_neg,
                                       const int *d_row_index_pos,
                                       const int *d_row_index_neg,
                                       int col_begin, int col_end, int device,
                                       void *stream, tcsc_gpu_plan **out);
int tcsc_gpu_plan_is_packed(const tcsc_gpu_plan *plan);
int tcsc_gpu_plan_copy_w2(const tcsc_gpu_plan *plan, void *d_dst, size_t bytes, void *stream);

/* ---- saved images: image -> packed plan, image -> TCSC, host packing
 * tcsc_gpu_plan_copy_w2 writes an image out; these take one back in.  The image
 * is the layout documented at tcsc_gpu_plan_enable_w2, tcsc_gpu_w2_image_bytes(
 * rows, cols) bytes, and must be canonical: no code 3, and code 1 at every
 * padding position (k >= rows, column >= cols).  Every image the library writes
 * is; copy_w2 round trips and the byte-for-byte invariant above depend on it.
 *
 * tcsc_gpu_plan_create_packed_image / _device: a packed plan from an image in
 * host memory (copied H2D) or on `device` (copied D2D).  `rows` is K, `cols` the
 * plan's own column count, col_begin >= 0 only labels info.col_begin (how a
 * column shard's image is reloaded).  The plan owns a copy and never adopts the
 * caller's pointer; the call synchronises `stream`.  The plan is the one
 * tcsc_gpu_plan_create_packed builds for the same W: is_packed 1, has_w2 1,
 * has_i8 0, device_bytes == tcsc_gpu_w2_image_bytes(rows, cols) exactly,
 * mfma_min_M 17, n_chunks 0, the same routing, reserve, workspace and refusals,
 * and copy_w2 returns the bytes that went in.  k_w2_check validates the copy and
 * counts it (one thread per dword, grid-stride; integer adds and one 64-bit
 * integer atomic per workgroup, so no order of execution shows): info.n_pos /
 * n_neg / nnz are the +1 / -1 weights of the image.  They equal the counts of
 * the plan the TCSC
 * arrays gave whenever W has no cancelling +1/-1 pair at one position (such a
 * pair is two entries there and weight 0 here).
 * TCSC_E_ARG with a message naming the call, *out NULL and no HIP call for: a
 * NULL image or out, rows < 1 or >= 2^22, cols < 1, col_begin < 0, bytes !=
 * tcsc_gpu_w2_image_bytes(rows, cols), a reference-order request.  TCSC_E_ARG
 * and no plan (nothing stays allocated) when the image holds a code 3 or
 * non-canonical padding; the message says which.
 *
 * tcsc_gpu_w2_to_tcsc: a device image -> the TCSC arrays of the rows x cols
 * matrix it encodes, on the current device, by tcsc_gpu_from_dense's two-call
 * protocol: with d_row_index_* NULL it writes d_col_start_* (cols + 1 offsets
 * from 0) and *n_pos / *n_neg; with them allocated to those sizes it fills them
 * too.  Bit for bit what tcsc_from_dense gives for that dense matrix: rows
 * ascending inside every column.  Integer counters only (k_w2_unpack: per
 * column and 256-k block counts, an exclusive scan, then every dword writes its
 * entries behind those of the dwords before it in k order); no atomics in the
 * fill, so every output position is determined by the image alone.  The image
 * must not change between the two calls of a pair.  The same validation and
 * host-side refusals as above, except that the summation order is not asked
 * (TCSC arrays serve either order); a sign with 2^31 entries or more is
 * TCSC_E_ARG (tcsc_t offsets are int).  Allocates scratch and synchronises
 * `stream`, as tcsc_gpu_from_dense does.
 *
 * tcsc_gpu_w2_from_tcsc_host / tcsc_gpu_w2_to_tcsc_host: the same two
 * conversions in host code, with no HIP call: they work where there is no
 * device.  The first writes the image of W[:, col_begin:col_end) into `image`
 * with k_w2_from_tcsc's semantics and bytes: a +1 and a -1 at one position
 * cancel, unsorted columns are accepted; TCSC_E_ARG for a position whose summed
 * weight is outside {-1, 0, +1}, a row outside [0, K), a col_start that is no
 * range, K >= 2^22, an empty column range or a wrong `bytes`.  The second
 * returns a new tcsc_t (free it with tcsc_free) with tcsc_gpu_w2_to_tcsc's
 * arrays, or NULL with tcsc_gpu_last_error() set on an invalid image or
 * arguments.
 *
 * Out of scope: a multi-layer checkpoint format (one image is one plan), packed
 * transposed plans, fp32 or bf16 calls on a packed plan, int8 Y, and a
 * host-pointer sgemm on images. */
int tcsc_gpu_plan_create_packed_image(const void *image, size_t bytes, int rows, int cols,
                                      int col_begin, int device, void *stream, tcsc_gpu_plan **out);
int tcsc_gpu_plan_create_packed_image_device(const void *d_image, size_t bytes, int rows, int cols,
                                             int col_begin, int device, void *stream, tcsc_gpu_plan **out);
int tcsc_gpu_w2_to_tcsc(const void *d_image, size_t bytes, int rows, int cols,
                        int *d_col_start_pos, int *d_col_start_neg,
                        int *d_row_index_pos, int *d_row_index_neg,
                        int *n_pos, int *n_neg, void *stream);
int tcsc_gpu_w2_from_tcsc_host(const tcsc_t *W, int col_begin, int col_end, void *image, size_t bytes);
tcsc_t *tcsc_gpu_w2_to_tcsc_host(const void *image, size_t bytes, int rows, int cols);

/* ---- the quantizer fused into the int8 decode call -------------
 * Token generation through the int8 path is tcsc_gpu_quantize_rows_i8 followed
 * by tcsc_gpu_sgemm_i8: two launches per layer, an int8 copy of X written and
 * read back, and fp32 rows only.  tcsc_gpu_sgemm_q8 takes the activations as
 * they are, fp32 or bf16, and where it pays runs both steps in one launch.
 *
 * tcsc_gpu_sgemm_q8:
 *   dX     : M x K row-major, contiguous; xtype TCSC_X_F32: floats, TCSC_X_BF16:
 *            bf16 bit patterns (16 bits each); any alignment of the element type
 *   dXq    : M x K bytes of scratch the caller owns (see below)
 *   dScale : M floats, always written: the quantizer's scales
 *   dB, dY, M, ldy, variant, a, stream : exactly as in tcsc_gpu_sgemm_i8
 * The contract is an equality of bits: dY and dScale hold what
 * tcsc_gpu_quantize_rows_i8 (xtype TCSC_X_BF16: tcsc_gpu_quantize_rows_i8_bf16)
 * into (dXq, dScale) followed by tcsc_gpu_sgemm_i8 on the same plan under the
 * same environment give -- on every plan that takes int8 calls (ordinary,
 * packed, column shards, transposed), at every M, for every variant and `a`.
 * Asynchronous on `stream`, capturable, and no workspace beyond the int8
 * call's: tcsc_gpu_plan_reserve and tcsc_gpu_plan_workspace are unchanged.
 *
 * Routing: the int8 route is the one tcsc_gpu_launch_info_i8 reports.  The call
 * is FUSED when that route is TCSC_PATH_DECODE and tcsc_gpu_quant_fuse_pays says
 * 1 or $TCSC_QFUSE=1 is set ($TCSC_QFUSE is read per call: 0 never fuses, 1
 * fuses on every decode route, unset follows the rule).  Fused, one kernel
 * (k_decode8q) finds the row maxima, writes dScale, quantizes X on the way into
 * its MFMA fragments with the quantizer's own arithmetic (one shared function)
 * and runs k_decode8's loop and epilogue; dXq is not touched and may be NULL.
 * Not fused, the library launches the quantizer into dXq and then the int8
 * call (two launches, three where k_pack8 runs); dXq must then be non-NULL:
 * TCSC_E_ARG otherwise, answered like every other argument check (a NULL plan,
 * X, scale, B or Y, xtype other than 0 or 1, M < 0, ldy < cols, a bad variant)
 * before any HIP call, with a message naming the call.
 * tcsc_gpu_launch_info_q8 reports the path, the K slices and whether a call of
 * M rows of that xtype is fused.
 *
 * tcsc_gpu_quant_fuse_pays (host arithmetic: no plan, no device): a fused
 * workgroup reads all of X twice from the L2 (the row maxima, then the values
 * it quantizes) and quantizes M K values itself, where k_decode8 reads the M K
 * bytes of the int8 copy once.  With W the workgroups of the launch
 * (ceil(ceil(N/16) / T), T the tiles per workgroup of k_decode8's grid rule on
 * 256 CUs) the rule is
 *   1 <= M <= 4 and W M K <= 2^23, for either xtype
 * -- where the fused call was measured no slower than the two launches, in a
 * replayed graph and eagerly (profiles/q8_bench.json: up to
 * M = 2 at 8192 x 8192 and M = 4 at 4096 x 4096, 2560 x 6912 and 6912 x 2560;
 * it loses at every M >= 8 measured).  0 for M < 1, M > 16, K < 1, N < 1 or an
 * xtype other than 0 or 1.
 *
 * tcsc_gpu_quantize_rows_i8_bf16: tcsc_gpu_quantize_rows_i8 on bf16 bit
 * patterns: each value is widened to fp32 (exact) and then takes the same
 * formula, so the results are those of the fp32 quantizer on the widened X.
 * The same guarantees and argument checks.
 *
 * Out of scope: int8 Y; fusing the quantizer into k_pack8 at M >= 17; a
 * host-pointer version. */
enum tcsc_xtype { TCSC_X_F32 = 0, TCSC_X_BF16 = 1 };
int tcsc_gpu_quantize_rows_i8_bf16(const void *dX_bf16, int M, int K, void *dXq, float *dScale, void *stream);
int tcsc_gpu_sgemm_q8(const tcsc_gpu_plan *plan, const void *dX, int xtype, void *dXq, float *dScale,
                      const float *dB, float *dY, int M, int ldy, int variant, float a, void *stream);
int tcsc_gpu_launch_info_q8(const tcsc_gpu_plan *plan, int M, int xtype, int *path, int *slices, int *fused);
int tcsc_gpu_quant_fuse_pays(int M, int K, int N, int xtype);

/* ---- int8 calls: per-column weight scales and a bf16 Y ---------
 * A ternarized weight is beta T with T in {-1, 0, +1}, beta one number per
 * tensor or one per output column, and the layer that follows reads bf16.  With
 * the calls above that is a zero bias, then mul_(beta), add_(bias), the
 * activation and a conversion: three or four launches and as many passes over an
 * fp32 Y beside a kernel of a few microseconds.  These two calls finish the
 * layer in the launches the int8 call already has.
 *
 * tcsc_gpu_sgemm_i8_out: tcsc_gpu_sgemm_i8, and tcsc_gpu_sgemm_q8_out:
 * tcsc_gpu_sgemm_q8, with
 *   dColScale : cols floats c[j] (the plan's slice, as dB), or NULL for all ones
 *   dY, ytype : TCSC_Y_F32: floats; TCSC_Y_BF16: bf16 bit patterns (16 bits
 *               each), which need 2-byte alignment only
 *   ldy       : the pitch of Y in elements of its type, >= cols
 * and every other argument exactly as in the call it extends.  With S the exact
 * i32 sum, s[m] the row scale (NULL: one), c[j] and b[j]:
 *   v = fl(fl(float(S) * s[m]) * c[j])      two multiplies, in this order
 *   v = fl(v + b[j])                        never contracted with a multiply
 *   v = v < 0 ? a * v : v                   the PReLU variants
 *   Y[m, j] = v                             TCSC_Y_F32
 *   Y[m, j] = bf16(v)                       TCSC_Y_BF16: round to nearest even
 *                                           on the fp32 bits -- for every finite
 *                                           v and +-inf what a conversion of
 *                                           the fp32 Y gives; a NaN stays a NaN
 * x * 1.0f == x, so (NULL, TCSC_Y_F32) gives the bits of tcsc_gpu_sgemm_i8 /
 * _q8, which are these calls with those two arguments.  The arithmetic is one
 * function shared by k_gemm8, k_gemm8w2, k_reduce_i8, k_decode8 and k_decode8q:
 * the same bits on every route, tile shape and K split, packed or ordinary
 * plan, fused quantizer or not.  Only rows < M and columns < cols are written:
 * a bf16 store never touches a 2-byte element outside them (column `cols` of an
 * odd cols, the element before an odd-aligned Y); four columns go out as one
 * 8-byte store only where Y is 8-byte aligned and ldy % 4 == 0.
 *
 * Routes: a call whose int8 route (tcsc_gpu_launch_info_i8 / _q8) is
 * TCSC_PATH_DECODE or TCSC_PATH_MFMA -- every call on a packed plan, and calls
 * on ordinary plans wherever the router picks those paths.  Where the route is
 * the gather or the small-M path, (NULL, TCSC_Y_F32) is the call as it was and
 * anything else returns TCSC_E_ARG before any HIP call, with a message naming
 * the call and the path: those paths finish in fp32 kernels shared with
 * tcsc_gpu_sgemm.  Routing, $TCSC_DECODE, $TCSC_QFUSE, $TCSC_W2GEMM,
 * $TCSC_MFMA_WGS, the fusing rule, the workspace, tcsc_gpu_plan_reserve and the
 * launch_info queries are unchanged: the calls allocate nothing once the
 * workspace covers M and can be captured.  The 2^22-row pieces of a packed plan
 * advance Y by the element size of its type.
 * On top of the checks of the calls they extend, TCSC_E_ARG with a message
 * naming the call and no HIP call for: ytype other than 0 or 1, a NULL plan, a
 * NULL dY, a NULL dB (these four whatever M is).
 *
 * Out of scope: int8 Y; column scales and a bf16 Y on the gather and small-M
 * routes and on the fp32 and bf16 calls; a host-pointer version. */
enum tcsc_ytype { TCSC_Y_F32 = 0, TCSC_Y_BF16 = 1 };
int tcsc_gpu_sgemm_i8_out(const tcsc_gpu_plan *plan, const void *dXq, const float *dScale,
                          const float *dColScale, const float *dB, void *dY, int ytype,
                          int M, int ldy, int variant, float a, void *stream);
int tcsc_gpu_sgemm_q8_out(const tcsc_gpu_plan *plan, const void *dX, int xtype, void *dXq,
                          float *dScale, const float *dColScale, const float *dB, void *dY,
                          int ytype, int M, int ldy, int variant, float a, void *stream);

/* ---- RMSNorm in the int8 call ----------------------------------
 * Every ternary linear of a BitNet-style model reads quant(RMSNorm(x) gamma).
 * These calls move the norm into the launches the int8 call already has.
 *
 * The arithmetic is pinned (csrc/tcsc_norm.h), every step one correctly rounded
 * fp32 operation, never contracted.  For a row x[0 .. K), bf16 widened exactly:
 *   ss     the sum of fl(x[k] x[k]) in an order that depends on K alone: 512
 *          partials, element k in partial (k >> 3) & 511, each partial summed
 *          in ascending k from +0, then the tree p[c] = fl(p[c] + p[c + s]) for
 *          s = 256, 128, .., 1
 *   r      mean = fl(ss / float(K)); r = fl(1 / fl(sqrt(fl(mean + eps))))
 *   xn[k]  fl(fl(x[k] r) gamma[k]); dGamma NULL = all ones, the same bits
 * and then the quantizer of tcsc_gpu_quantize_rows_i8 on xn.  Inputs must be
 * finite with squares that do not overflow; otherwise the values are
 * unspecified.  Rows >= M and elements >= K are never read.
 *
 * tcsc_gpu_rmsnorm_rows: dXn (M x K floats) = xn, and dRinv[m] = r where dRinv
 *   is not NULL.  dX: M x K, xtype as in tcsc_gpu_sgemm_q8; dGamma: K floats or
 *   NULL.  Every pointer needs the alignment of its element type only.
 * tcsc_gpu_quantize_rows_i8_norm: the bits of tcsc_gpu_rmsnorm_rows into an fp32
 *   Xn followed by tcsc_gpu_quantize_rows_i8 of Xn, in one launch at every M.
 * tcsc_gpu_sgemm_q8_norm: tcsc_gpu_sgemm_q8_out with the norm in front.  dY and
 *   dScale hold the bits of tcsc_gpu_rmsnorm_rows, tcsc_gpu_quantize_rows_i8 and
 *   tcsc_gpu_sgemm_i8_out on the same plan and environment: at every M, variant,
 *   a, ytype and column scale, on packed, ordinary, column-shard and transposed
 *   plans.
 *
 * Routing: the int8 route is what tcsc_gpu_launch_info_i8 reports.  The call is
 * FUSED -- one launch of the norm form of k_decode8q -- when that route is
 * TCSC_PATH_DECODE and tcsc_gpu_norm_fuse_pays says 1 or $TCSC_QFUSE=1 is set
 * ($TCSC_QFUSE as in tcsc_gpu_sgemm_q8: 0 never fuses, unset follows the rule);
 * dXq is then not touched and may be NULL.  Otherwise the call is
 * tcsc_gpu_quantize_rows_i8_norm into dXq (non-NULL) and the int8 call: two
 * launches, three where k_pack8 runs.  dColScale and ytype as in
 * tcsc_gpu_sgemm_q8_out, the refusal on the gather and small-M routes included.
 * Workspace, tcsc_gpu_plan_reserve and capture are unchanged; no call allocates
 * or synchronises.  tcsc_gpu_launch_info_q8_norm reports the path, the K slices
 * and whether a call of M rows of that xtype is fused.
 *
 * On top of the checks of tcsc_gpu_sgemm_q8_out, TCSC_E_ARG with a message
 * naming the call and no HIP call for: an eps that is not finite or not > 0,
 * K < 1, an xtype other than 0 or 1, a NULL dXn in tcsc_gpu_rmsnorm_rows.
 *
 * tcsc_gpu_norm_fuse_pays (host arithmetic: no plan, no device): 0 for every
 * argument, as measured.  Every fused workgroup sweeps all of X three times
 * (the squares, the maxima of xn, the values it quantizes) where
 * tcsc_gpu_sgemm_q8's sweeps it twice, and the launch it saves is the norm form of
 * the quantizer, which reads a row of up to 8192 elements once.  The rule keeps
 * tcsc_gpu_quant_fuse_pays's form, 1 <= M <= M0 and W M K <= V0 with W the
 * workgroups of the launch, and its fit is M0 = 0: in replayed graphs
 * (profiles/norm_bench.json; packed plans at 4096 x 4096,
 * 8192 x 8192, 2560 x 6912 and 6912 x 2560, M = 1, 2, 4, 8, 16, fp32 and bf16 x)
 * the fused call beat the library's own two launches beyond the run's spread
 * only at a few points of M <= 2 with bf16 x, by 6 % at the most, and was
 * level or slower everywhere else, down to a quarter of the speed at M = 16 --
 * also at M = 1 with bf16 x on shapes whose W M K lie between those of the
 * wins, so no bound on W M K separates the two.  So without
 * $TCSC_QFUSE=1 the call is always the norm form of the quantizer followed by
 * the int8 call, and the fused form is there for a caller who has measured a
 * point of their own.
 *
 * Out of scope: a bf16 gamma; LayerNorm with a mean; writing xn out of the
 * fused call; the norm on the fp32, bf16 and plain int8 calls; int8 Y; a
 * host-pointer version. */
int tcsc_gpu_rmsnorm_rows(const void *dX, int xtype, const float *dGamma, float eps,
                          int M, int K, float *dXn, float *dRinv /* may be NULL */, void *stream);
int tcsc_gpu_quantize_rows_i8_norm(const void *dX, int xtype, const float *dGamma, float eps,
                                   int M, int K, void *dXq, float *dScale, void *stream);
int tcsc_gpu_sgemm_q8_norm(const tcsc_gpu_plan *plan, const void *dX, int xtype,
                           const float *dGamma, float eps, void *dXq, float *dScale,
                           const float *dColScale, const float *dB, void *dY, int ytype,
                           int M, int ldy, int variant, float a, void *stream);
int tcsc_gpu_launch_info_q8_norm(const tcsc_gpu_plan *plan, int M, int xtype,
                                 int *path, int *slices, int *fused);
int tcsc_gpu_norm_fuse_pays(int M, int K, int N, int xtype);   /* host arithmetic */

/* ---- Gated FFN in the int8 call ---------------------------------
 * The FFN of a BitNet-style block is down(quant(subnorm(act(gate(x)) * up(x)))).
 * The gate and up projections share X, its row scales and its quantizer, and
 * their outputs meet element by element: these calls compute
 *   Y = act(X Wg) * (X Wu)
 * on two plans, so that a whole FFN is two library calls -- a gated call into a
 * bf16 Y, and tcsc_gpu_sgemm_q8_norm on that Y.
 *
 * The arithmetic is pinned; every step is one rounded fp32 operation and no step
 * is contracted with another.  With Sg, Su the exact i32 sums against the gate
 * and up weights, s[m] the row scale, cg, cu the column scales (NULL: all ones)
 * and bg, bu the biases:
 *   g = fl(fl(fl(float(Sg) s[m]) cg[j]) + bg[j])      tcsc_gpu_sgemm_i8_out's value,
 *   u = fl(fl(fl(float(Su) s[m]) cu[j]) + bu[j])      no PReLU
 *   TCSC_GLU_RELU2:  r = g < 0 ? 0 : g;  h = fl(fl(r r) u)
 *   TCSC_GLU_SILU:   h = fl(fl(g / fl(1 + expf(-g))) u)    IEEE division, the
 *                    device math library's expf (1 ulp); a very negative
 *                    finite g gives expf = inf and g / inf = -0, g = -inf
 *                    gives -inf / inf = NaN
 *   Y[m, j] = h (TCSC_Y_F32) or h rounded to bf16, nearest even (TCSC_Y_BF16)
 * Every route gives the same bits: TCSC_GLU_RELU2 those of two
 * tcsc_gpu_sgemm_i8_out calls into fp32 followed by torch's
 * relu(g).square() * u (and .to(bfloat16)).  Inputs are finite.  Only rows < M
 * and columns < cols are written, with the store rules of tcsc_gpu_sgemm_i8_out.
 *
 * gate, up: two plans with the same rows (K) and cols (H) on one device, each
 *   holding the 2-bit image: a packed plan, or an ordinary plan after
 *   tcsc_gpu_plan_enable_w2.  Two plans rather than one of 2 H columns: H needs
 *   no alignment, the image format and its save / load do not change, and the
 *   plans of existing layers serve.
 * dG: the caller's scratch for the gate values, M x H floats at pitch H, as dXq
 *   is the quantizer's.  Needed where the route is TCSC_PATH_MFMA; untouched,
 *   and allowed to be NULL, where it is TCSC_PATH_DECODE.
 * dY: M x ldy of ytype, ldy >= H in elements.
 *
 * Routes (tcsc_gpu_launch_info_glu), by M and, from 17 to 64 rows, the two
 * plans' decode_rows_multi setting ("gated and grouped calls at 17 .. 64 rows"
 * below; by default everything above 16 rows is the MFMA route) --
 * the cost models, $TCSC_PATH and $TCSC_DECODE are not asked:
 *   M <= 16  TCSC_PATH_DECODE: one launch (k_decode8g) that streams both images
 *            against one set of X fragments.  tcsc_gpu_sgemm_q8_glu runs the
 *            quantizer inside it (k_decode8qg: *fused = 1) where
 *            tcsc_gpu_glu_fuse_pays says so or $TCSC_QFUSE=1 is set ($TCSC_QFUSE=0:
 *            never); otherwise the quantizer (with the norm: its norm form) into
 *            dXq, then k_decode8g.
 *   17 <= M <= 64, where both plans' setting admits M: TCSC_PATH_DECODE too, one
 *            launch (k_decode8gr) on the quantized X; dG untouched.
 *   M >= 17  otherwise TCSC_PATH_MFMA: k_pack8 once, then k_gemm8w2 twice on the gate
 *            plan's workspace (slabs included: *slices is the K split of each) --
 *            the gate half through the plain epilogue into dG, the up half
 *            through the gated one.  tcsc_gpu_plan_reserve(gate, max_M) covers it;
 *            a call on a smaller workspace grows it first, as tcsc_gpu_sgemm_i8
 *            does.  Once reserved, no call allocates or synchronises, and all
 *            can be captured.
 *
 * tcsc_gpu_sgemm_q8_glu takes an fp32 or bf16 X (xtype as in tcsc_gpu_sgemm_q8),
 * writes the row scales to dScale and uses dXq as tcsc_gpu_sgemm_q8 does (NULL
 * allowed where the call is fused).  eps == 0.0f exactly, with a NULL dGamma,
 * means no norm; any other eps is checked as tcsc_gpu_sgemm_q8_norm checks it
 * and the RMSNorm of that call runs in front of the quantizer.
 *
 * tcsc_gpu_glu_fuse_pays (host arithmetic: no plan, no device): the rule of
 * tcsc_gpu_quant_fuse_pays with the gated launch's own workgroup count W =
 * ceil(ceil(H / 16) / TG): 1 for 1 <= M <= 4 and W M K <= 2^23; with norm != 0
 * tcsc_gpu_norm_fuse_pays's, which is 0 everywhere.  tcsc_gpu_launch_info_glu
 * reports *fused for a call without the norm.
 *
 * TCSC_E_ARG with a message naming the call, before any HIP call, for: a NULL
 * plan, dY, bias or X; a plan without the 2-bit image; plans whose K, cols or
 * device differ; an act or ytype out of range; a NULL dG on the MFMA route; a
 * NULL dXq where the call is not fused; dGamma given with eps == 0; ldy < cols.
 *
 * Out of scope: one GEMM launch over both images on the MFMA route;
 * gating on the gather and small-M routes and on the fp32 and bf16 calls; an
 * int8 Y; other gate activations; a host-pointer version. */
enum tcsc_glu_act { TCSC_GLU_RELU2 = 0, TCSC_GLU_SILU = 1 };
int tcsc_gpu_sgemm_i8_glu(const tcsc_gpu_plan *gate, const tcsc_gpu_plan *up,
                          const void *dXq, const float *dScale,
                          const float *dColScaleG, const float *dBG,
                          const float *dColScaleU, const float *dBU,
                          float *dG /* may be NULL on the decode route */, void *dY, int ytype,
                          int M, int ldy, int act, void *stream);
int tcsc_gpu_sgemm_q8_glu(const tcsc_gpu_plan *gate, const tcsc_gpu_plan *up,
                          const void *dX, int xtype, const float *dGamma, float eps,
                          void *dXq, float *dScale,
                          const float *dColScaleG, const float *dBG,
                          const float *dColScaleU, const float *dBU,
                          float *dG /* may be NULL on the decode route */, void *dY, int ytype,
                          int M, int ldy, int act, void *stream);
int tcsc_gpu_launch_info_glu(const tcsc_gpu_plan *gate, const tcsc_gpu_plan *up, int M, int xtype,
                             int *path, int *slices, int *fused);
int tcsc_gpu_glu_fuse_pays(int M, int K, int N, int xtype, int norm);   /* host arithmetic */

/* ---- Grouped int8 call: several matrices on one X ---------------
 * The Q, K and V projections of an attention block read the same
 * quant(RMSNorm(x) gamma), the same row scales and the same int8 X, as do any
 * projections that share an input.  These calls run up to TCSC_GROUP_MAX of them
 * as one: member i's output is, bit for bit, what
 *   tcsc_gpu_sgemm_i8_out(members[i].plan, dXq, dScale, dColScale_i, dB_i, dY_i,
 *                         ytype, M, ldy_i, TCSC_VARIANT_BASIC, 0, stream)
 * writes -- that call stays the definition of the arithmetic -- and the q8 form
 * equals the norm, the quantizer and the i8 form, as tcsc_gpu_sgemm_q8 /
 * tcsc_gpu_sgemm_q8_norm do.  There is no PReLU on this call.
 *
 * members: count (1 .. TCSC_GROUP_MAX) of
 *   plan       a plan that holds the 2-bit image (a packed plan, or an ordinary
 *              one after tcsc_gpu_plan_enable_w2).  All members have the same
 *              rows (K) and device; the column counts are free, with no
 *              alignment to the 16-column tile.
 *   dColScale  cols floats, NULL: all ones;  dB: cols floats
 *   dY, ldy    M x ldy of the call's ytype, ldy >= cols in elements.  The members'
 *              dY may point into one tensor at different column offsets with a
 *              common pitch (a fused qkv tensor): the store rules are
 *              tcsc_gpu_sgemm_i8_out's, any element alignment.  Overlapping
 *              outputs are the caller's mistake and are not checked.
 * A group of one gives the single call's bits with the single call's grid.
 *
 * Routes (tcsc_gpu_launch_info_group), by M and, from 17 to 64 rows, the members'
 * decode_rows_multi setting ("gated and grouped calls at 17 .. 64 rows" below,
 * DESIGN.md §28; by default everything above 16 rows is the MFMA route) -- the
 * cost models, $TCSC_PATH and $TCSC_DECODE are not asked:
 *   M <= 16  TCSC_PATH_DECODE: one launch (k_decode8m) whose grid is the
 *            concatenation of the members' workgroups: member i owns
 *            ceil(ceil(cols_i / 16) / T) consecutive workgroups of T column tiles
 *            each, T being one value per launch -- 4 above 8 rows, 2 above 4, else
 *            1, halved while the whole grid W = sum_i ceil(tiles_i / T) is below
 *            the CU count.  tcsc_gpu_sgemm_q8_group without the norm runs the
 *            quantizer inside that launch (k_decode8qm: *fused = 1) where
 *            tcsc_gpu_group_fuse_pays says so or $TCSC_QFUSE=1 is set
 *            ($TCSC_QFUSE=0: never); otherwise the quantizer into dXq, then
 *            k_decode8m.  The fused kernel has no norm form (the norm inside the
 *            decode launch lost at 37 of 40 measured points): a
 *            grouped call with the norm always runs the norm form of the
 *            quantizer into dXq and then k_decode8m, whatever $TCSC_QFUSE says,
 *            and needs dXq.
 *   17 <= M <= 64, where every member's setting admits M: TCSC_PATH_DECODE too,
 *            the quantizer (with the norm: its norm form) into dXq and then one
 *            launch (k_decode8mr) on k_decode8m's grid.
 *   M >= 17  otherwise TCSC_PATH_MFMA: the quantizer (with the norm: its norm form) once,
 *            k_pack8 once into the first member's workspace, and k_gemm8w2 once
 *            per member, each GEMM's K-split slabs in its own plan's workspace
 *            (slices[i] is member i's K split).  tcsc_gpu_plan_reserve(plan,
 *            max_M) on every member covers the call; a smaller workspace is grown
 *            first, as every int8 call does.  Once reserved, no call allocates or
 *            synchronises, and all can be captured.
 *
 * tcsc_gpu_sgemm_q8_group takes an fp32 or bf16 X (xtype as in tcsc_gpu_sgemm_q8),
 * writes the row scales to dScale and uses dXq as tcsc_gpu_sgemm_q8 does (NULL
 * allowed where the call is fused).  eps == 0.0f exactly, with a NULL dGamma,
 * means no norm; any other eps is checked as tcsc_gpu_sgemm_q8_norm checks it
 * and the RMSNorm of that call runs in front of the quantizer.
 *
 * tcsc_gpu_group_fuse_pays (host arithmetic: no plan, no device): the rule of
 * tcsc_gpu_quant_fuse_pays with the grouped launch's workgroup count W: 1 for
 * 1 <= M <= 4 and W M K <= 2^23; 0 with norm != 0.  For one member it is
 * tcsc_gpu_quant_fuse_pays.  tcsc_gpu_launch_info_group reports *fused for a
 * call without the norm; slices receives count ints.
 *
 * TCSC_E_ARG with a message naming the call and, where it applies, the member's
 * index, before any HIP call, for: count outside 1 .. TCSC_GROUP_MAX; NULL
 * members; a ytype or xtype out of range; a NULL plan, dB or dY of a member; a
 * member plan without the 2-bit image; members whose K or device differ; ldy <
 * cols; M < 0; a NULL X; on the q8 form a bad eps, dGamma given with eps == 0,
 * a NULL dScale, and a NULL dXq where the call is not fused.  M == 0 is TCSC_OK.
 *
 * Out of scope: one GEMM launch over all images on the MFMA route; a norm form of the
 * fused grouped kernel; PReLU or gating on this call; the gather and small-M
 * routes; a host-pointer version. */
#define TCSC_GROUP_MAX 4
typedef struct tcsc_gpu_group_member {
    const tcsc_gpu_plan *plan;   /* holds the 2-bit image */
    const float *dColScale;      /* cols floats, NULL: ones */
    const float *dB;             /* cols floats */
    void *dY;                    /* M x ldy of the call's ytype */
    int ldy;                     /* >= plan cols, in elements */
} tcsc_gpu_group_member;

int tcsc_gpu_sgemm_i8_group(const tcsc_gpu_group_member *members, int count,
                            const void *dXq, const float *dScale,
                            int ytype, int M, void *stream);
int tcsc_gpu_sgemm_q8_group(const tcsc_gpu_group_member *members, int count,
                            const void *dX, int xtype, const float *dGamma, float eps,
                            void *dXq, float *dScale,
                            int ytype, int M, void *stream);
int tcsc_gpu_launch_info_group(const tcsc_gpu_group_member *members, int count, int M, int xtype,
                               int *path, int *slices /* count ints */, int *fused);
int tcsc_gpu_group_fuse_pays(int M, int K, const int *cols, int count, int xtype, int norm); /* host arithmetic */

/* ---- Residual add in the int8 epilogue: Y = R + X W --------------
 * The output and down projections of a transformer block end in a skip
 * connection, h = h + proj(x).  These calls add the residual where the value
 * still sits in registers, instead of a second launch that reads Y and R and
 * writes Y again.  With S the exact i32 sum of row m and column j:
 *   v = fl(fl(fl(float(S) * dScale[m]) * dColScale[j]) + dB[j])
 *                               tcsc_gpu_sgemm_i8_out's value, TCSC_VARIANT_BASIC
 *   r = dR[m * ldr + j]         of ytype; a bf16 r is widened exactly
 *   y = fl(v + r)               one rounded fp32 add, never contracted
 *   dY[m * ldy + j] = y (TCSC_Y_F32), or y rounded to nearest even (TCSC_Y_BF16)
 * R has the type of Y: the residual stream is what the call writes.  There is
 * no PReLU, no `variant` and no `a` on these calls.
 *
 * Every route gives the same bits -- decode and MFMA, both GEMM tile shapes,
 * every K split, packed and ordinary plans, the quantizer fused or not, the
 * norm in front or not:
 *   fp32 Y   tcsc_gpu_sgemm_i8_out into an fp32 Y0, then the fp32 add Y0 + R;
 *   bf16 Y   bf16(Y0 + float(R)) with that fp32 Y0: ONE rounding to bf16.
 * This is not what a bf16 layer followed by a bf16 add gives: that composition
 * rounds v to bf16 first and the sum a second time, and differs from this call
 * in the last bit of many elements.
 *
 * In place.  dR == dY with ldr == ldy is allowed: every output element is read
 * and written by the same thread, the read first, and elements past the matrix
 * are neither read nor written.  dR == dY with ldr != ldy is refused.  Any other
 * overlap of R, Y, X and Xq is the caller's mistake and is not checked.
 *
 * Reads and stores.  Only rows < M and columns < cols of R are read; R is never
 * written unless it is Y.  The store rules of tcsc_gpu_sgemm_i8_out hold for Y.
 * A lane's four adjacent columns travel as one access where ldy % 4 == 0 and Y
 * is aligned to four of its elements and, on these calls, ldr % 4 == 0 and R is
 * aligned to four elements as well; otherwise element by element, each guarded.
 *
 * tcsc_gpu_sgemm_q8_res is tcsc_gpu_sgemm_q8_out -- with a norm,
 * tcsc_gpu_sgemm_q8_norm -- followed by the add: X is fp32 or bf16 (xtype), the
 * row scales are written to dScale and dXq is used as those calls use it (NULL
 * allowed where the call is fused).  eps == 0.0f exactly, with a NULL dGamma,
 * means no norm (tcsc_gpu_sgemm_q8_glu's convention); any other eps is checked
 * as tcsc_gpu_sgemm_q8_norm checks it.
 *
 * Routing, fusing, workspace and capture are those of the calls extended: the
 * route is what tcsc_gpu_launch_info_i8 / _q8 / _q8_norm report for the plan and
 * M; the quantizer is fused under tcsc_gpu_quant_fuse_pays (with the norm:
 * tcsc_gpu_norm_fuse_pays); $TCSC_DECODE, $TCSC_QFUSE, $TCSC_W2GEMM and
 * $TCSC_MFMA_WGS keep their meaning.  The calls are served on TCSC_PATH_DECODE
 * and TCSC_PATH_MFMA; where M routes to the gather or the small-M path they
 * return TCSC_E_ARG with a message naming the call and the path, as the _out
 * calls do for a typed Y.  After tcsc_gpu_plan_reserve(plan, max_M) a call of
 * M <= max_M allocates nothing, does not synchronise and can be captured; a
 * captured in-place call applied n times adds n products to R.
 *
 * TCSC_E_ARG with a message naming the call, before any HIP call, in this
 * order: (q8 form) an xtype out of range, dGamma given with eps == 0, a bad
 * eps; a ytype out of range; a NULL plan; a NULL dY or dB; a NULL dR;
 * ldr < cols; dR == dY with ldr != ldy; then the checks of the calls extended
 * (M < 0, ldy < cols, a NULL X or dScale, a NULL dXq where not fused).
 *
 * Out of scope: a residual on the gated and grouped calls; a residual of
 * another type than Y's; PReLU with a residual; the gather and small-M routes;
 * the next layer's norm-quantizer behind the add; a host-pointer version. */
int tcsc_gpu_sgemm_i8_res(const tcsc_gpu_plan *plan, const void *dXq, const float *dScale,
                          const float *dColScale, const float *dB,
                          const void *dR, int ldr, void *dY, int ytype,
                          int M, int ldy, void *stream);
int tcsc_gpu_sgemm_q8_res(const tcsc_gpu_plan *plan, const void *dX, int xtype,
                          const float *dGamma, float eps, void *dXq, float *dScale,
                          const float *dColScale, const float *dB,
                          const void *dR, int ldr, void *dY, int ytype,
                          int M, int ldy, void *stream);

/* ---- int8 decode up to 64 rows: a per-plan setting ---------------
 * k_decode8r is k_decode8 with two or four 16-row tiles per workgroup: one
 * launch that reads X in place and streams the 2-bit image once, every expanded
 * fragment of the image feeding one MFMA per row tile.  Same sums, same
 * epilogue (row and column scales, bias, PReLU or the residual, fp32 or bf16
 * Y, R == Y in place): the bits of the MFMA route at the same M.  No workspace,
 * no allocation, no synchronisation: capturable.
 *
 * tcsc_gpu_plan_set_decode_rows(plan, rows): the most rows an int8 call on this
 * plan takes to TCSC_PATH_DECODE.  rows is 16 .. 64 or TCSC_DECODE_ROWS_AUTO;
 * the default is 16, which routes every call as before.  With a number, int8
 * calls of 16 < M <= rows take the decode path; with AUTO, those for which
 * tcsc_gpu_decode_rows_pays(M, K, cols, CUs of the device) says 1, asked per
 * call.  TCSC_E_ARG for a NULL plan, any other value, or a plan without the
 * 2-bit image.  On an ordinary plan $TCSC_DECODE=0 still vetoes the path and a
 * pinned TCSC_PATH_MFMA still wins; M <= 16 is untouched in every respect.
 * Setting it allocates and frees nothing and does not synchronise, and it is no
 * part of a saved plan.  tcsc_gpu_plan_decode_rows reads it back (TCSC_E_ARG,
 * which is no value of the setting, for a NULL plan).
 *
 * Served: tcsc_gpu_sgemm_i8, _i8_out, _i8_res, and behind the quantizer's own
 * launch tcsc_gpu_sgemm_q8, _q8_out, _q8_norm, _q8_res -- above 16 rows a q8
 * call is never fused, whatever $TCSC_QFUSE says; tcsc_gpu_launch_info_i8 /
 * _q8 / _q8_norm report the route.  The gated and grouped calls do not read
 * this setting: they have one of their own, decode_rows_multi (below, §28).
 *
 * Workspace: tcsc_gpu_plan_workspace(plan, M, TCSC_PATH_AUTO) reports the need
 * of the route the setting gives, 0 on the decode route.  tcsc_gpu_plan_reserve
 * sizes every M > 16 for the MFMA route whatever the setting is: the setting
 * may change afterwards, and the gated and grouped calls borrow the workspace.
 *
 * tcsc_gpu_decode_rows_pays (host arithmetic: no plan, no device): the rule
 * fitted to profiles/decode_rows_bench.json,
 *   17 <= M <= 32 and K N <= 2^26
 * -- with two row tiles the launch beat k_pack8 + k_gemm8w2 at every measured
 * shape (2560^2 .. 8192^2: 1.2x to 2.2x); with four (M >= 33) it won at the
 * square shapes and lost at 2560 x 6912 and 6912 x 2560, so the rule is 0
 * there and 33 .. 64 rows are an explicit opt-in.  num_cus is not read today.
 *
 * tcsc_gpu_launch_info_decode: what a decode launch of M rows on this plan
 * would run, whether or not the setting routes M there: *row_tiles (1 up to 16
 * rows, 2 up to 32, 4 up to 64), *col_tiles (column tiles of 16 per workgroup:
 * 1, 2 or 4) and *workgroups (the grid).  TCSC_E_ARG for a NULL argument, a plan
 * without the image, M < 1 or M > 64.
 *
 * Out of scope: the quantizer inside the launch above 16 rows; more than 64
 * rows.  (The gated and grouped calls above 16 rows: §28, below.) */
#define TCSC_DECODE_ROWS_AUTO (-1)
int tcsc_gpu_plan_set_decode_rows(tcsc_gpu_plan *plan, int rows);
int tcsc_gpu_plan_decode_rows(const tcsc_gpu_plan *plan);
int tcsc_gpu_decode_rows_pays(int M, int K, int N, int num_cus);
int tcsc_gpu_launch_info_decode(const tcsc_gpu_plan *plan, int M, int *row_tiles, int *col_tiles,
                                long long *workgroups);

/* ---- gated and grouped calls at 17 .. 64 rows: a second per-plan setting
 * k_decode8gr and k_decode8mr are k_decode8g and k_decode8m with two or four
 * 16-row tiles per workgroup, as k_decode8r is k_decode8's: one launch on an
 * int8 X that streams the 2-bit images once, without a workspace and without
 * dG, and gives the bits of the MFMA route at the same M.
 *
 * tcsc_gpu_plan_set_decode_rows_multi(plan, rows): the most rows a gated or
 * grouped call takes to TCSC_PATH_DECODE as far as this plan is concerned.  rows
 * is 16 .. 64 or TCSC_DECODE_ROWS_AUTO; the default is 16, which routes every
 * call as before.  A call of 16 < M <= 64 rows decodes when EVERY plan of the
 * call -- gate and up, or all members -- admits M: a plan set to a number
 * admits M <= rows, a plan set to AUTO admits M where the call's own rule
 * (tcsc_gpu_glu_rows_pays(M, K, H, CUs), or tcsc_gpu_group_rows_pays over the
 * members' column counts) says 1, asked per call.  Otherwise the call routes
 * as before.  $TCSC_PATH, $TCSC_DECODE and the cost models are not asked, as
 * on these calls everywhere; M <= 16 is untouched in every respect; the
 * decode_rows setting of §27 is not read.  TCSC_E_ARG for a NULL plan, any
 * other value, or a plan without the 2-bit image.  Setting it writes one int:
 * it allocates and frees nothing, does not synchronise, and is no part of a
 * saved plan.  tcsc_gpu_plan_decode_rows_multi reads it back (TCSC_E_ARG, which
 * is no value of the setting, for a NULL plan).
 *
 * On the decode route: tcsc_gpu_launch_info_glu / _group report *path =
 * TCSC_PATH_DECODE, slices of 1 and, above 16 rows, *fused = 0; dG may be NULL
 * and is untouched (the "NULL dG on the MFMA route" refusal follows the route,
 * not M); the q8 forms above 16 rows run the quantizer's launch (with a norm:
 * its norm form) and then the kernel -- never fused, whatever $TCSC_QFUSE says
 * -- and need dXq.  tcsc_gpu_plan_reserve is unchanged: it sizes M > 16 for the
 * MFMA route, because the setting may change afterwards.
 *
 * tcsc_gpu_glu_rows_pays, tcsc_gpu_group_rows_pays (host arithmetic: no plan, no
 * device): the rules fitted to profiles/multi_rows_bench.json
 * (tools/multi_rows_bench.py) alone,
 *   gated    17 <= M <= 64 and K H <= 2^26
 *   grouped  17 <= M <= 64 and K (sum of the members' columns) <= 8192 * 10240
 * -- the one launch beat both samples of the MFMA route at all 36 measured
 * points of 17 .. 64 rows, with two row tiles and with four (gated 1.15x to
 * 2.40x at 2560 x 6912, 4096^2, 8192^2; grouped 1.19x to 3.45x at 2560 +
 * 640 + 640, 3 x 4096 and 8192 + 1024 + 1024 columns), the margin falling with
 * the size of W, so each rule stops at the largest shape measured.  0 elsewhere:
 * M <= 16, M > 64, K < 1 or >= 2^22, a column count < 1, a count outside
 * 1 .. TCSC_GROUP_MAX.  num_cus is not read today.  The default setting stays
 * 16: AUTO is the caller's choice.
 *
 * tcsc_gpu_launch_info_glu_decode / _group_decode: what a decode launch of M
 * rows (1 .. 64) of these plans would run, whether or not M routes there:
 * *row_tiles (1, 2 or 4), *col_tiles (per workgroup; gated: TG of each image,
 * 2 or 1 at two row tiles and 1 at four; grouped: 4, 2 or 1 at two row tiles, 2
 * or 1 at four -- from the most eight accumulator tiles allow, halved while the
 * grid is below the CU count) and *workgroups.  TCSC_E_ARG as the calls' own
 * plan checks, for a NULL output and for M outside 1 .. 64.
 *
 * Out of scope: the quantizer or the norm inside the launch above 16 rows; more
 * than 64 rows; one MFMA GEMM launch over several images; a residual or PReLU
 * on the gated and grouped calls. */
int tcsc_gpu_plan_set_decode_rows_multi(tcsc_gpu_plan *plan, int rows);  /* 16 .. 64 or TCSC_DECODE_ROWS_AUTO */
int tcsc_gpu_plan_decode_rows_multi(const tcsc_gpu_plan *plan);
int tcsc_gpu_glu_rows_pays(int M, int K, int H, int num_cus);                       /* host arithmetic */
int tcsc_gpu_group_rows_pays(int M, int K, const int *cols, int count, int num_cus); /* host arithmetic */
int tcsc_gpu_launch_info_glu_decode(const tcsc_gpu_plan *gate, const tcsc_gpu_plan *up, int M,
                                    int *row_tiles, int *col_tiles, long long *workgroups);
int tcsc_gpu_launch_info_group_decode(const tcsc_gpu_group_member *members, int count, int M,
                                      int *row_tiles, int *col_tiles, long long *workgroups);

/* Device-side tcsc_from_dense: dense K x N row-major float matrix on the
 * device -> TCSC arrays on the device, bit-exact with the reference builder
 * (tcsc.c:6-66).  Two calls: first with the four output pointers NULL to
 * get n_pos / n_neg (col_start arrays are still written), then with the
 * index arrays allocated.  The matrix must not change between the two calls
 * of a pair (the second call reuses the first call's per-tile counts when it
 * follows it directly with the same matrix, shape and col_start arrays; the
 * index arrays are never written past the counted sizes either way).
 * Synchronises `stream`. */
int tcsc_gpu_from_dense(const float *d_dense, int rows, int cols,
                        int *d_col_start_pos, int *d_col_start_neg,
                        int *d_row_index_pos, int *d_row_index_neg,
                        int *n_pos, int *n_neg, void *stream);

/* Dense baseline, the device counterpart of the
 * reference's gemm_basic (dense/dense.c:64-77) that the harness times for
 * its "TCSC vs Dense" line (main.cpp:379-391):
 *   Y[m, n] = act(sum_k X[m,k] * W[k,n] + B[n])
 * with W the DENSE K x N row-major float matrix (the ternary W before
 * tcsc_from_dense), computed as an fp32 rocBLAS SGEMM plus a bias/PReLU
 * epilogue kernel.  act as in tcsc_gpu_sgemm (PReLU for the PRELU
 * variants).  dX: M x K row-major; dY: M rows of pitch ldy >= N.
 * Asynchronous on `stream`. */
int tcsc_gpu_dense_sgemm(const float *dX, const float *dW, const float *dB,
                         float *dY, int M, int N, int K, int ldy, int variant,
                         float a, void *stream);

/* ---- Backward pass ------------------------------------------
 * For Y = act(X.W + b) with upstream gradient G = dL/dY:
 *   dZ = G masked by the PReLU derivative, db = column sums of dZ
 *        (tcsc_gpu_prelu_backward)
 *   dX = dZ . W^T                          (tcsc_gpu_sgemm_t on a transposed plan)
 * W^T of a TCSC matrix is again a TCSC matrix, so dX runs on an ordinary plan
 * built from the transposed index arrays: every kernel family, the cost model,
 * reserve and split K serve it unchanged.  There is no host-pointer version. */

/* Device-side transposition of the index structure: from the TCSC arrays of
 * W (rows x cols, on the current device, absolute offsets) to those of
 * W[:, col_begin:col_end)^T, a matrix of col_end - col_begin rows and `rows`
 * columns: d_t_csp / d_t_csn get rows + 1 offsets starting at 0, d_t_rip /
 * d_t_rin the range's n_pos = csp[col_end] - csp[col_begin] and n_neg column
 * indices j - col_begin, ascending inside every output column -- bit for bit
 * what tcsc_from_dense (tcsc.c:6-66) gives for the dense transposed slice.
 * Deterministic: integer counters only, and every output column is sorted, so
 * no order of execution shows in the output.  The order inside an input
 * column does not matter (unsorted input columns are accepted); a col_start
 * that is no range or a row outside [0, rows) is TCSC_E_ARG.  An empty range,
 * rows == 0 or no entries still write the offsets (all zero).  The row index
 * pointers may be NULL where the range has no entry of that sign.  Allocates
 * scratch and synchronises `stream`, as tcsc_gpu_from_dense does. */
int tcsc_gpu_transpose_index(int rows, int cols,
                             const int *d_col_start_pos, const int *d_col_start_neg,
                             const int *d_row_index_pos, const int *d_row_index_neg,
                             int col_begin, int col_end,
                             int *d_t_col_start_pos, int *d_t_col_start_neg,
                             int *d_t_row_index_pos, int *d_t_row_index_neg,
                             void *stream);

/* The plan of W[:, col_begin:col_end)^T: uploads the column range as
 * tcsc_gpu_plan_create does, transposes it on the device and builds an
 * ordinary plan from the result: info.rows = col_end - col_begin, info.cols =
 * W->rows, info.col_begin = 0.  Everything that takes a plan works on it
 * unchanged; it honours tcsc_gpu_set_order, $TCSC_ORDER and $TCSC_PATH at
 * creation as any plan does.  It also owns a zero bias of info.cols floats
 * (counted in device_bytes) for tcsc_gpu_sgemm_t.  A second plan costs what
 * the first does: about 8 bytes per nonzero plus the per-chunk headers, plus
 * the CSC copy and, for denser W, the bf16 image. */
int tcsc_gpu_plan_create_transposed(const tcsc_t *W, int col_begin, int col_end,
                                    int device, void *stream, tcsc_gpu_plan **out);

/* Same, from raw TCSC arrays of W that already live on `device` (the layout
 * tcsc_gpu_plan_create_device takes).  Nothing crosses PCIe. */
int tcsc_gpu_plan_create_transposed_device(int rows, int cols,
                                           const int *d_col_start_pos,
                                           const int *d_col_start_neg,
                                           const int *d_row_index_pos,
                                           const int *d_row_index_neg,
                                           int col_begin, int col_end, int device,
                                           void *stream, tcsc_gpu_plan **out);

/* dX[m, k] = sum_j G[m, j] * W[k, col_begin + j] for m < M, k < K:
 *   dG  : M x (col_end - col_begin) row-major, contiguous (the plan's rows)
 *   dDX : M rows with pitch ldx >= K floats; columns beyond K are not touched
 * tcsc_gpu_sgemm on the transposed plan with TCSC_VARIANT_SPARSE_GEMM and the
 * plan's zero bias, with every guarantee of tcsc_gpu_sgemm (asynchronous,
 * allocation-free once reserved, safe to capture).  Column shards of W give
 * partial dX's that the caller adds.  TCSC_E_ARG on a plan that no
 * _transposed constructor made. */
int tcsc_gpu_sgemm_t(const tcsc_gpu_plan *tplan, const float *dG, float *dDX,
                     int M, int ldx, void *stream);

/* The elementwise half of the layer's backward, for m < M, j < N:
 *   dDZ[m, j] = dY[m, j] < 0.0f ? a * dG[m, j] : dG[m, j]
 *   dDB[j]    = sum_m dDZ[m, j]   (fp32, of the rounded dDZ values)
 * dY is the forward's OUTPUT and the predicate is the forward's own
 * (tcsc.c:162), so the mask is exact: NaN, -0.0 and +0.0 in dY pass dG
 * through.  dY NULL: identity activation (dDZ = dG).  dDZ may alias dG, or be
 * NULL when only dDB is wanted; dDB may be NULL.  dG, dY and dDZ have their
 * own row pitches (ldg, ldy, lddz >= N floats; 16-byte accesses when every
 * pointer is 16-B aligned and every pitch a multiple of 4, scalar otherwise).
 * dDB is summed in a fixed order (each of 32 row-lanes its rows m = r, r + 32,
 * ... in ascending m, then the lanes pairwise), so it is bitwise reproducible;
 * no float atomics, no scratch, no allocation, no synchronisation: safe to
 * capture.  M == 0 writes dDB = 0.  Asynchronous on `stream`. */
int tcsc_gpu_prelu_backward(const float *dG, int ldg, const float *dY, int ldy, float a,
                            float *dDZ, int lddz, float *dDB, int M, int N, void *stream);

/* Message for the last failing call on this thread ("" if none). */
const char *tcsc_gpu_last_error(void);

/* Drop every device copy the host-pointer API cached (all tcsc_t's). */
void tcsc_gpu_cache_clear(void);

/* Number of GPUs the host-pointer API (sparse/tcsc.h) spreads columns over:
 * min(visible devices, $TCSC_NUM_GPUS if set).  `tcsc_gpu_set_num_shards`
 * overrides the count of column blocks (blocks are dealt round-robin over
 * the devices; >devices is allowed and is how the multi-block path is
 * exercised on a single GPU). 0 restores the default. */
int tcsc_gpu_num_shards(void);
void tcsc_gpu_set_num_shards(int shards);

/* The host-pointer API (sparse/tcsc.h, include/sparse_gemm.h) runs in EXACT
 * mode by default: every call sums each output in dense.c gemm_basic's order
 * (y = 0; y += X*W over ascending k; y += B; then the PReLU for the PReLU
 * variants) -- the fast order with K never split, never the MFMA path -- so
 * its outputs equal the reference harness's own oracle bit for bit
 * (main.cpp:307-366 checks tcsc_sgemm_basic / _optimized against it with an
 * absolute 1e-4).  $TCSC_HOST_FAST=1 (read per call) lets host calls take the
 * device API's fastest paths instead (MFMA, split K): within the fp32 bound
 * of the exact sums, not bit-equal to gemm_basic. */

/* Diagnostic build flags of the loaded library: 0 for the product build;
 * bits 1 TCSC_ABLATION, 2 TCSC_NODMA, 4 TCSC_STAMPS, 8 TCSC_TRACE (timing-only
 * builds of tools/ab.mk whose outputs are wrong by design). */
int tcsc_gpu_build_flags(void);

#ifdef __cplusplus
}
#endif

#endif /* TCSC_AMD_TCSC_GPU_H */
