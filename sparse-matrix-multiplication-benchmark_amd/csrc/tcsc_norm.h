// tcsc_norm.h -- the arithmetic of the RMSNorm in front of the int8 quantizer
// (DESIGN.md §22), shared by every kernel that normalises a row of X:
// k_rmsnorm_rows and the norm form of k_quant_rows_i8 (tcsc_mfma.hip) and the
// norm form of k_decode8q (tcsc_decode.hip).  One definition, so the kernels
// give the same bits.  Every step is one correctly rounded fp32 operation and
// none is contracted into an fma: the functions below switch contraction off
// for themselves (HIP's __fmul_rn / __fadd_rn are a plain * and + that the
// compiler may fuse, and its __fsqrt_rn is the approximate native square root,
// so neither is used here; x / y and __builtin_sqrtf are correctly rounded in a
// default HIP build).
//
// For a row x[0 .. K), bf16 widened exactly:
//   ss    the sum of fl(x[k] * x[k]) in a fixed order that depends on K alone:
//         kNormPartials = 512 partials; element k belongs to partial
//         (k >> 3) & 511 (groups of kNormGroup = 8 consecutive elements -- one
//         16-B load of bf16, two of fp32 -- dealt round-robin); a partial adds
//         its squares in ascending k, starting from +0; the 512 partials are
//         folded by the tree p[c] = fl(p[c] + p[c + s]), s = 256, 128, .., 1.
//         Squares are >= +0, so elements that are not there (k >= K) may be
//         left out or added as +0: the bits are the same.
//   r     mean = fl(ss / float(K)); r = fl(1 / fl(sqrt(fl(mean + eps))))
//   xn[k] fl(fl(x[k] * r) * gamma[k]); a NULL gamma is all ones (the second
//         multiply is skipped: the same bits)
// and then tcsc_quant.h on xn.
//
// A team of NT threads (a power of two, NT <= 512) sums a row: thread `sub`
// owns the 512 / NT partials sub + NT j, visits the groups sub, sub + NT, ..
// and folds the strides 256 .. NT in registers (norm_ss_thread); the strides
// below NT are between threads: through the LDS down to 32 and by xor shuffles
// inside a half-wave (fl(a + b) = fl(b + a): a butterfly leaves every lane the
// tree's bits).
#pragma once
#include <hip/hip_runtime.h>

#include "tcsc_xsrc.h"

namespace tcsc {

constexpr int kNormPartials = 512;
constexpr int kNormGroup = 8;

// fl(p + fl(x * x))
__device__ __forceinline__ float norm_sq_add(float p, float x) {
#pragma clang fp contract(off)
    const float sq = x * x;
    return p + sq;
}

// fl(a + b), never part of an fma
__device__ __forceinline__ float norm_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// r of a row from its sum of squares
__device__ __forceinline__ float norm_rinv(float ss, int K, float eps) {
#pragma clang fp contract(off)
    const float mean = __fdiv_rn(ss, (float)K);
    const float t = mean + eps;
    return __fdiv_rn(1.0f, __builtin_sqrtf(t));
}

// xn = fl(fl(x * r) * g), and the form without gamma
__device__ __forceinline__ float norm_apply(float x, float r, float g) {
#pragma clang fp contract(off)
    const float t = x * r;
    return t * g;
}
__device__ __forceinline__ float norm_apply(float x, float r) {
#pragma clang fp contract(off)
    return x * r;
}

// the N (4 or 8) values x[k0 .. k0 + N) of a 16-B piece turned into xn in place;
// gamma (if any) is 16-B aligned and k0 a multiple of 4: 16-B loads of gamma
template <int N>
__device__ __forceinline__ void norm_piece(float (&w)[N], float r, const float* __restrict__ gamma, int k0) {
    static_assert(N % 4 == 0, "whole 16-B pieces of gamma");
    if (gamma) {
#pragma unroll
        for (int d = 0; d < N / 4; ++d) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + k0 + 4 * d);
            w[4 * d] = norm_apply(w[4 * d], r, g.x);
            w[4 * d + 1] = norm_apply(w[4 * d + 1], r, g.y);
            w[4 * d + 2] = norm_apply(w[4 * d + 2], r, g.z);
            w[4 * d + 3] = norm_apply(w[4 * d + 3], r, g.w);
        }
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) w[e] = norm_apply(w[e], r);
    }
}

// group g of a row (elements 8 g .. 8 g + 7, those below K) added to partial p
// in ascending k.  VEC: XSrc<TX>::vec_ok, so a 16-B piece lies wholly below K.
template <typename TX, bool VEC>
__device__ __forceinline__ float norm_add_group(float p, const TX* __restrict__ row, int K, int g) {
    using XS = XSrc<TX>;
    const int k0 = kNormGroup * g;
    if constexpr (VEC) {
#pragma unroll
        for (int h = 0; h < kNormGroup / XS::kVec; ++h) {
            if (k0 + XS::kVec * h >= K) break;  // fp32 at K % 8 == 4: half a group
            float f[XS::kVec];
            XS::unpack(*reinterpret_cast<const uint4*>(row + k0 + XS::kVec * h), 1.0f, f);
#pragma unroll
            for (int e = 0; e < XS::kVec; ++e) p = norm_sq_add(p, f[e]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < kNormGroup; ++e)
            if (k0 + e < K) p = norm_sq_add(p, XS::conv(row[k0 + e], 1.0f));
    }
    return p;
}

// the 8 values of group g, zeros for k >= K (a zero adds nothing to a partial and
// stays zero through norm_apply without gamma)
template <typename TX, bool VEC>
__device__ __forceinline__ void norm_load_group(const TX* __restrict__ row, int K, int g, float (&x)[kNormGroup]) {
    using XS = XSrc<TX>;
    const int k0 = kNormGroup * g;
#pragma unroll
    for (int e = 0; e < kNormGroup; ++e) x[e] = 0.0f;
    if constexpr (VEC) {
#pragma unroll
        for (int h = 0; h < kNormGroup / XS::kVec; ++h) {
            if (k0 + XS::kVec * h >= K) break;
            float f[XS::kVec];
            XS::unpack(*reinterpret_cast<const uint4*>(row + k0 + XS::kVec * h), 1.0f, f);
#pragma unroll
            for (int e = 0; e < XS::kVec; ++e) x[XS::kVec * h + e] = f[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < kNormGroup; ++e)
            if (k0 + e < K) x[e] = XS::conv(row[k0 + e], 1.0f);
    }
}

// the 8 values of group g turned into xn in place.  VEC: K % 4 == 0 and gamma (if
// any) 16-B aligned, so a half group takes one 16-B load of gamma or lies past K.
template <bool VEC>
__device__ __forceinline__ void norm_group_xn(float (&x)[kNormGroup], float r, const float* __restrict__ gamma, int K,
                                              int g) {
    const int k0 = kNormGroup * g;
    if constexpr (VEC) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (k0 + 4 * h >= K) break;
            float w[4] = {x[4 * h], x[4 * h + 1], x[4 * h + 2], x[4 * h + 3]};
            norm_piece<4>(w, r, gamma, k0 + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[4 * h + e] = w[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < kNormGroup; ++e)
            x[e] = gamma && k0 + e < K ? norm_apply(x[e], r, gamma[k0 + e]) : norm_apply(x[e], r);
    }
}

// Thread `sub` of a team of NT: its partials over the whole row, folded over the
// strides 256 .. NT.  What returns is node `sub` of the tree at width NT.
template <typename TX, int NT, bool VEC>
__device__ __forceinline__ float norm_ss_thread(const TX* __restrict__ row, int K, int sub) {
    static_assert(NT >= 1 && NT <= kNormPartials && (NT & (NT - 1)) == 0, "a power of two up to 512");
    constexpr int P = kNormPartials / NT;
    float p[P];
#pragma unroll
    for (int j = 0; j < P; ++j) p[j] = 0.0f;
    const int ngroups = (K + kNormGroup - 1) / kNormGroup;
    for (int g0 = sub; g0 < ngroups; g0 += kNormPartials) {  // rounds of 4096 elements
#pragma unroll
        for (int j = 0; j < P; ++j)
            if (g0 + NT * j < ngroups) p[j] = norm_add_group<TX, VEC>(p[j], row, K, g0 + NT * j);
    }
#pragma unroll
    for (int s = P / 2; s >= 1; s >>= 1)
#pragma unroll
        for (int j = 0; j < s; ++j) p[j] = norm_add(p[j], p[j + s]);
    return p[0];
}

// The strides NT / 2 .. 1 of a team of NT >= 32 consecutive threads (the team of
// thread tid starts at tid & ~(NT - 1)): every thread leaves its node in
// part[tid] (blockDim.x floats), reads the NT / 32 nodes of its lane of the
// half-wave, folds them, and the half-wave's 32 lanes finish by xor shuffles.
// Every thread of the team returns ss.  All threads of the workgroup call this
// (one __syncthreads inside; a second one before part[] is written again is
// the caller's).
template <int NT>
__device__ __forceinline__ float norm_ss_team(float node, float* part, int tid) {
    static_assert(NT >= 32 && NT <= kNormPartials && (NT & (NT - 1)) == 0, "whole half-waves");
    constexpr int H = NT / 32;
    part[tid] = node;
    __syncthreads();
    const int base = (tid & ~(NT - 1)) + (tid & 31);
    float w[H];
#pragma unroll
    for (int i = 0; i < H; ++i) w[i] = part[base + 32 * i];
#pragma unroll
    for (int s = H / 2; s >= 1; s >>= 1)
#pragma unroll
        for (int i = 0; i < s; ++i) w[i] = norm_add(w[i], w[i + s]);
    float v = w[0];
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) v = norm_add(v, __shfl_xor(v, d, 64));  // stays inside the half-wave
    return v;
}

}  // namespace tcsc
