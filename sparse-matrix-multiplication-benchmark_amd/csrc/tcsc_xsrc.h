// tcsc_xsrc.h -- device side of the activation type (kernels only; the host's
// descriptor table is kXTypes in tcsc_api.cpp).  XSrc<TX> is the one place that
// knows how a piece of an X row becomes floats: TX = float (tcsc_gpu_sgemm),
// uint16_t (bf16 bit patterns, tcsc_gpu_sgemm_bf16) or int8_t with a per-row
// scale (tcsc_gpu_sgemm_i8).  k_transpose and k_small_m derive their staging
// geometry from kVec and call nothing else of the type.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace tcsc {

template <typename TX>
struct XSrc {
    static constexpr bool kF32 = std::is_same<TX, float>::value, kScaled = std::is_same<TX, int8_t>::value;
    static_assert(kF32 || kScaled || std::is_same<TX, uint16_t>::value, "X is fp32, bf16 bit patterns or int8");
    static constexpr int kVec = 16 / (int)sizeof(TX);  // elements of one 16-byte load: 4 / 8 / 16

    // 16-byte loads need whole pieces in every row and aligned rows
    __host__ __device__ static bool vec_ok(const TX* X, int K) {
        return K % kVec == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    }

    // the factor of row m: read by the int8 form only (null = one)
    __device__ static float row_scale(const float* __restrict__ scale, int m) {
        if constexpr (kScaled)
            return scale ? scale[m] : 1.0f;
        else
            return 1.0f;
    }

    // one element: fp32 as it is, bf16 widened (bits << 16), int8 fl(s * float(x))
    __device__ static float conv(TX x, float s) {
        if constexpr (kF32)
            return x;
        else if constexpr (kScaled)
            return __fmul_rn(s, (float)x);
        else
            return __uint_as_float((uint32_t)x << 16);
    }

    // the kVec elements of a 16-byte piece, in memory order
    __device__ static void unpack(const uint4& v, float s, float (&f)[kVec]) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        constexpr int kPer = kVec / 4;  // elements per 32-bit word
#pragma unroll
        for (int e = 0; e < kVec; ++e) {
            if constexpr (kF32)
                f[e] = __uint_as_float(w[e]);
            else
                f[e] = conv((TX)(w[e / kPer] >> (32 / kPer * (e % kPer))), s);
        }
    }
};

}  // namespace tcsc
