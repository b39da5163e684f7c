// tcsc_i8_out.h -- the epilogue arithmetic of the int8 call,
// shared by every kernel that turns an exact i32 sum into Y: k_gemm8 and
// k_reduce_i8 (tcsc_mfma.hip), k_decode8 and k_decode8q (tcsc_decode.hip).  One
// definition, so the paths give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace tcsc {

// act(fl(fl(float(S) * s) + b)): one conversion (round to nearest), one
// multiply, one add that must not contract with it, then the PReLU.
template <bool PRELU>
__device__ __forceinline__ float i8_out(int S, float s, float b, float a) {
    // (__fmul_rn / __fadd_rn are plain * and + to hipcc, which would fuse them)
#pragma clang fp contract(off)
    const float p = (float)S * s;
    const float v = p + b;
    return PRELU ? ((v < 0.0f) ? a * v : v) : v;
}

}  // namespace tcsc
