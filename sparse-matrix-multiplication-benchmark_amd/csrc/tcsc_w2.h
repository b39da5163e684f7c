// tcsc_w2.h -- one dword of the 2-bit image of W (tcsc_internal.h, "int8 decode
// path") into the four dwords of a lane's v_mfma_i32_16x16x64_i8 fragment: the
// one definition behind k_decode8, k_decode8q (tcsc_decode.hip) and k_gemm8w2
// (tcsc_mfma.hip).  Kernels only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tcsc {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// Fragment dword d as the codes c = w + 1 of its four weights, bytes 0 .. 2:
// one shift and one mask.
__device__ __forceinline__ uint32_t w2_code(uint32_t p, int d) { return (p >> (2 * d)) & 0x03030303u; }

// The fragment of codes as they are.  A kernel that multiplies by these takes
// sum q c and subtracts the row sums (k_decode8).
__device__ __forceinline__ i32x4 w2_codes(uint32_t p) {
    return i32x4{(int)w2_code(p, 0), (int)w2_code(p, 1), (int)w2_code(p, 2), (int)w2_code(p, 3)};
}

// The fragment of signed weights: one v_perm_b32 per dword takes each code as
// the selector into the bytes ff, 00, 01 (codes 0, 1, 2 -> -1, 0, +1), so the
// MFMAs give S = sum q w itself (k_gemm8w2).  Dword by dword, not through
// w2_codes: built from the vector of codes, k_gemm8w2's 128 x 128 shapes took
// two more VGPRs and every M = 2048 point measured 0.3-0.9 % slower.
__device__ __forceinline__ i32x4 w2_frag(uint32_t p) {
    i32x4 b;
#pragma unroll
    for (int d = 0; d < 4; ++d) b[d] = (int)__builtin_amdgcn_perm(0x000100ffu, 0x000100ffu, w2_code(p, d));
    return b;
}

}  // namespace tcsc
