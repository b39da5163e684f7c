// tcsc_quant.h -- the arithmetic of the per-row absmax quantizer (DESIGN.md §16,
// §20), shared by every kernel that turns a row of X into int8: k_quant_rows_i8
// (tcsc_mfma.hip, fp32 and bf16 X) and k_decode8q (tcsc_decode.hip).  One
// definition, so the kernels give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace tcsc {

// scale = amax / 127 and inv = 127 / amax, each one correctly rounded division;
// a row without a positive maximum (all zeros) gets 0 for both
__device__ __forceinline__ void quant_scales(float amax, float& scale, float& inv) {
    const bool zero = !(amax > 0.0f);
    scale = zero ? 0.0f : __fdiv_rn(amax, 127.0f);
    inv = zero ? 0.0f : __fdiv_rn(127.0f, amax);
}

// q = clamp(rint(fl(x * inv)), -127, 127): one rounded multiply, round to
// nearest even, the clamp, the conversion
__device__ __forceinline__ int quant_i8(float x, float inv) {
    return (int)fminf(fmaxf(rintf(__fmul_rn(x, inv)), -127.0f), 127.0f);
}

}  // namespace tcsc
