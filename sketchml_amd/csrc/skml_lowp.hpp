// skml_lowp.hpp -- bf16 / fp16 bit patterns as the sparse compaction reads them: the exact widening
// to float and DenseDoubleGradient.toSparse's keep test (Maths.scala:8 EPS: |x| > 1e-8, NaN out,
// +-inf in) taken on the 16 bits themselves.  No device builtin appears here: the kernels of
// skml_sparse_compact.hip and the host program tests/sparse_lowp_check.cpp build the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SKML_LP_FN __host__ __device__ __forceinline__
#else
#define SKML_LP_FN inline
#endif

namespace skml {

constexpr uint32_t kEpsBelowBits = 0x322BCC77u;  // the largest float <= 1e-8 (Maths.scala:8 EPS)

// |x| > 1e-8 in double for a float x with bit pattern b: |x| > RD_f32(1e-8) on the magnitude bits,
// NaN excluded (magnitude bits above +inf's).
SKML_LP_FN bool keep_f32_bits(uint32_t b) {
    const uint32_t a = b & 0x7FFFFFFFu;
    return a > kEpsBelowBits && a <= 0x7F800000u;
}

// bf16 is the float's upper half: the widened magnitude is (h & 0x7FFF) << 16, which lies above
// kEpsBelowBits exactly when its upper half lies above kEpsBelowBits' (0x322B).
SKML_LP_FN bool keep_bf16_bits(uint16_t h) {
    const uint32_t a = h & 0x7FFFu;
    return a > (kEpsBelowBits >> 16) && a <= 0x7F80u;
}
// fp16's smallest subnormal is 2^-24 > 1e-8: every finite non-zero value is kept.
SKML_LP_FN bool keep_f16_bits(uint16_t h) {
    const uint32_t a = h & 0x7FFFu;
    return a != 0 && a <= 0x7C00u;
}

SKML_LP_FN uint32_t widen_bf16_bits(uint16_t h) { return (uint32_t)h << 16; }
// fp16 -> float bits in integer arithmetic.  The kernels widen the kept values with the device's
// conversion instruction (skml_device.hpp widen2), which gives the same bits for every pattern
// that is not a NaN; the keep test drops NaN before its value is looked at.
SKML_LP_FN uint32_t widen_f16_bits(uint16_t h) {
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 31u) return s | 0x7F800000u | (m << 13);
    if (e != 0u) return s | ((e + 112u) << 23) | (m << 13);
    if (m == 0u) return s;
    int k = 9;  // subnormal m * 2^-24: the top set bit of m becomes the hidden one
    while (!((m >> k) & 1u)) k--;
    return s | ((uint32_t)(k + 103) << 23) | ((m << (23 - k)) & 0x7FFFFFu);
}

}  // namespace skml
