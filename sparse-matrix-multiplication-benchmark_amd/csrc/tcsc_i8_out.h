// tcsc_i8_out.h -- the epilogue arithmetic of the int8 call (DESIGN.md §16,
// §21), shared by every kernel that turns an exact i32 sum into Y: k_gemm8,
// k_gemm8w2 and k_reduce_i8 (tcsc_mfma.hip), k_decode8 and k_decode8q
// (tcsc_decode.hip), and the gate of the gated forms (§24: k_decode8g,
// k_decode8qg, gemm8_store and k_reduce_i8 with GLU), and the residual add of
// the residual forms (§26).  One definition, so the paths give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "tcsc_internal.h"

namespace tcsc {

// act(fl(fl(fl(float(S) * s) * c) + b)): one conversion (round to nearest even), the
// row scale, the column scale, one add that must not contract with either
// multiply, then the PReLU.  A call without column scales passes c = 1.0f:
// x * 1.0f == x for every x, so its bits are those of the two-step form.
template <bool PRELU>
__device__ __forceinline__ float i8_out(int S, float s, float c, float b, float a) {
    // (__fmul_rn / __fadd_rn are plain * and + to hipcc, which would fuse them)
#pragma clang fp contract(off)
    const float p = (float)S * s;
    const float q = p * c;
    const float v = q + b;
    return PRELU ? ((v < 0.0f) ? a * v : v) : v;
}

// The gate of a gated call: g and u are i8_out<false> of the gate
// and up sums, act the run-time activation (enum tcsc_glu_act) as a uniform
// branch.  Every step is one rounded fp32 operation, none contracted:
//   kGluRelu2  r = g < 0 ? 0 : g;  fl(fl(r r) u)           torch relu(g).square() * u
//   kGluSilu   fl(fl(g / fl(1 + expf(-g))) u)              IEEE division, the math library's expf
// (a very negative finite g gives expf = inf, g / inf = -0 and a zero of the sign
// of -u; g = -inf gives -inf / inf, a NaN, as a NaN g does).
__device__ __forceinline__ float i8_glu(float g, float u, int act) {
#pragma clang fp contract(off)
    if (act == kGluRelu2) {
        const float r = g < 0.0f ? 0.0f : g;
        const float r2 = r * r;
        return r2 * u;
    }
    const float e = expf(-g);
    const float d = 1.0f + e;
    const float s = __fdiv_rn(g, d);
    return s * u;
}

// The residual add of a residual call: v is i8_out<false> of the
// sum and r the element of R, of Y's type and widened exactly (I8Y<TY>::get).
// One rounded fp32 add, whatever stands around it: fl(v + r).
__device__ __forceinline__ float i8_res(float v, float r) {
#pragma clang fp contract(off)
    const float y = v + r;
    return y;
}

// c[j] of a call (null: all ones)
__device__ __forceinline__ float i8_cscale(const float* __restrict__ c, int j) { return c ? c[j] : 1.0f; }

// fp32 -> bf16 bits, round to nearest even on the fp32 bits: torch's
// .to(torch.bfloat16) for every finite value and +-inf (a finite value within
// half a bf16 ulp of the largest rounds to inf there too); a NaN stays a NaN.
__device__ __forceinline__ uint16_t i8_bf16(float v) {
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// The Y element of a call: float (TCSC_Y_F32) or bf16 bits (TCSC_Y_BF16).
// put() stores one element and put4_nt() a lane's four adjacent columns as one
// non-temporal store (16 B of floats, 8 B of bf16; dst aligned to four
// elements): every store of either type goes through one of them, so a 2-byte
// element is never written as half of a wider store it does not wholly own.
// get() and get4() are the reads of a residual R of the same type (§26): one
// element, or a lane's four adjacent columns as one load (src aligned to four
// elements), widened to fp32 exactly.
template <typename TY>
struct I8Y;
template <>
struct I8Y<float> {
    static __device__ __forceinline__ void put(float* dst, float v) { *dst = v; }
    static __device__ __forceinline__ void put_nt(float* dst, float v) { __builtin_nontemporal_store(v, dst); }
    static __device__ __forceinline__ void put4_nt(float* dst, float v0, float v1, float v2, float v3) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(f32x4{v0, v1, v2, v3}, reinterpret_cast<f32x4*>(dst));
    }
    static __device__ __forceinline__ float get(const float* src) { return *src; }
    static __device__ __forceinline__ void get4(const float* src, float (&r)[4]) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const f32x4 q = *reinterpret_cast<const f32x4*>(src);
        r[0] = q[0], r[1] = q[1], r[2] = q[2], r[3] = q[3];
    }
};
template <>
struct I8Y<uint16_t> {
    static __device__ __forceinline__ void put(uint16_t* dst, float v) { *dst = i8_bf16(v); }
    static __device__ __forceinline__ void put_nt(uint16_t* dst, float v) {
        __builtin_nontemporal_store(i8_bf16(v), dst);
    }
    static __device__ __forceinline__ void put4_nt(uint16_t* dst, float v0, float v1, float v2, float v3) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 o = {(uint32_t)i8_bf16(v0) | (uint32_t)i8_bf16(v1) << 16,
                         (uint32_t)i8_bf16(v2) | (uint32_t)i8_bf16(v3) << 16};
        __builtin_nontemporal_store(o, reinterpret_cast<u32x2*>(dst));
    }
    static __device__ __forceinline__ float get(const uint16_t* src) { return __uint_as_float((uint32_t)*src << 16); }
    static __device__ __forceinline__ void get4(const uint16_t* src, float (&r)[4]) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 q = *reinterpret_cast<const u32x2*>(src);
        r[0] = __uint_as_float(q[0] << 16), r[1] = __uint_as_float(q[0] & 0xffff0000u);
        r[2] = __uint_as_float(q[1] << 16), r[3] = __uint_as_float(q[1] & 0xffff0000u);
    }
};

// The Y parameter of a kernel with a residual form: restrict-qualified as ever
// where there is no residual, and plain where there is one, because an
// in-place call passes one pointer as R and as Y (§26).
template <typename TY, bool RES>
using I8YPtr = std::conditional_t<RES, TY*, TY* __restrict__>;

}  // namespace tcsc
