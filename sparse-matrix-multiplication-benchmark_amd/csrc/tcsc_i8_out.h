// tcsc_i8_out.h -- the epilogue arithmetic of the int8 call (DESIGN.md §16,
// §21), shared by every kernel that turns an exact i32 sum into Y: k_gemm8,
// k_gemm8w2 and k_reduce_i8 (tcsc_mfma.hip), k_decode8 and k_decode8q
// (tcsc_decode.hip), and the gate of the gated forms (§24: k_decode8g,
// k_decode8qg, gemm8_store and k_reduce_i8 with GLU).  One definition, so the
// paths give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tcsc_internal.h"

namespace tcsc {

// act(fl(fl(fl(float(S) * s) * c) + b)): one conversion (round to nearest), the
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
// (a very negative g gives expf = inf, g / inf = -0 and a zero of u's sign).
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
};

}  // namespace tcsc
