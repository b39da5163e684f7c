// tcsc_quant.h -- the arithmetic of the per-row absmax quantizer (DESIGN.md §16,
// §20), shared by every kernel that turns a row of X into int8: k_quant_rows_i8
// (tcsc_mfma.hip, fp32 and bf16 X) and k_decode8q (tcsc_decode.hip).  One
// definition, so the kernels give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace tcsc {

// scale = amax / 127 and inv = 127 / amax, each one correctly rounded division;
// a row without a positive maximum (all zeros) gets 0 for both, and so does a
// row whose maximum is so small that fl(127 / amax) is +inf (amax <= 127 * 2^-128
// = 0x02FE0000, about 3.73e-37; every subnormal maximum is one): x * inf would turn the row's
// zeros into NaN and every other element into +-127 whatever its ratio to
// amax.  Such a row counts as a row of zeros: at most K * 3.8e-37 per output.
// The division is monotonic and 127 / (127 * 2^-128) is 2^128 exactly, so
// "fl(127 / amax) is inf or amax is not positive" is "not amax > 127 * 2^-128":
// one compare, where the rule for the all-zero row alone had one against 0.
constexpr float kQuantMinAmax = 0x1.fcp-122f;  // 127 * 2^-128
__device__ __forceinline__ void quant_scales(float amax, float& scale, float& inv) {
    const bool zero = !(amax > kQuantMinAmax);
    scale = zero ? 0.0f : __fdiv_rn(amax, 127.0f);
    inv = zero ? 0.0f : __fdiv_rn(127.0f, amax);
}

// q = clamp(rint(fl(x * inv)), -127, 127): one rounded multiply, round to
// nearest even, the clamp, the conversion
__device__ __forceinline__ int quant_i8(float x, float inv) {
    return (int)fminf(fmaxf(rintf(__fmul_rn(x, inv)), -127.0f), 127.0f);
}

}  // namespace tcsc
