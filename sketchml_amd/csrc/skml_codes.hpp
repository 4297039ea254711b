// skml_codes.hpp -- reading a dense payload's packed codes and its value table on the device:
// what the decode / decode-sum kernels (skml_dense.hip) and the fused optimiser step
// (skml_optim.hip) share.
#pragma once
#include "skml_device.hpp"

namespace skml {

__device__ __forceinline__ uint32_t read_code(const uint8_t* codes, int64_t e, int bits) {
    switch (bits) {
        case 8: return codes[e];
        case 16: return reinterpret_cast<const uint16_t*>(codes)[e];
        case 4: return (codes[e >> 1] >> ((e & 1) * 4)) & 15u;
        case 2: return (codes[e >> 2] >> ((e & 3) * 2)) & 3u;
        default: return (codes[e >> 3] >> (e & 7)) & 1u;
    }
}

// Quantizer.getValues()[b]: the bin's midpoint in double (Quantizer.java:39-47).
__device__ __forceinline__ double lut_value(const skml_dense_header* h, const double* sp, int b) {
    const int ns = h->bin_num - 1;
    if (b == 0) return 0.5 * (h->min + sp[0]);
    if (b == ns) return 0.5 * (sp[ns - 1] + h->max);
    return 0.5 * (sp[b - 1] + sp[b]);
}

// Fused decode of P payloads + sum in double (Gradient.sum adds doubles) + scale.  Payloads of at
// most kSumLutBins bins look their values up in an LDS table; wider ones (16-bit codes) compute
// the midpoint from the payload's splits, as k_decode does above kLutMax.
constexpr int kMaxSumPayloads = 16;
constexpr int kSumLutBins = 256;
constexpr int kSumChunk = 8;

#ifndef SKML_OCC_WAVES
#define SKML_OCC_WAVES 4  // waves per SIMD of the prefetching form, 8- and 16-bit codes (4 against 6 and 8: profiles/ab/r06_occ_waves.txt)
#endif
#ifndef SKML_OCC_WAVES_NARROW
// the same for 1-, 2- and 4-bit codes: a step then loads 1-4 bytes per payload and lane, so the
// codes need more waves in flight (C5's 2-bit sum ran 154 us at 6 and 253 us at 4, profiles/ab/r06_occ_narrow.txt)
#define SKML_OCC_WAVES_NARROW 6
#endif
#ifndef SKML_OCC_PER
#define SKML_OCC_PER 8  // elements per lane and step (A/B builds: 16)
#endif
constexpr int kOccPer = SKML_OCC_PER, kOccMaxP = 8;
static_assert(kOccPer == 8 || kOccPer == 16, "8 or 16 elements per lane");
// dynamic LDS of the P tables: what is left of the 64 KB a launch may take without opting in
// after the kernel's static array of code pointers
constexpr size_t kOccLdsMax = 64 * 1024 - sizeof(const uint8_t*) * kOccMaxP;
// code words one lane holds per payload and step of PER elements
template <int BITS, int PER = kOccPer>
constexpr int occ_words() { return PER * BITS >= 32 ? PER * BITS / 32 : 1; }
// The code loads go through a global (address space 1) pointer: the payloads' code pointers sit in
// LDS, and loads through a generic pointer would be flat loads, which count on lgkmcnt too, so the
// table lookups' LDS waits would also wait for the next step's prefetched codes.
#define SKML_G(T) const __attribute__((address_space(1))) T*
template <int BITS, int PER = kOccPer>
__device__ __forceinline__ void load_codes_occ(const uint8_t* codes_any, int64_t e0, uint32_t (&w)[occ_words<BITS, PER>()]) {
    SKML_G(uint8_t) codes = (SKML_G(uint8_t))codes_any;
    constexpr int kBytes = PER * BITS / 8;  // e0 is a multiple of PER: aligned to kBytes
    const int64_t b0 = e0 * BITS / 8;
    typedef uint32_t u32x4_g __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2_g __attribute__((ext_vector_type(2)));
    if constexpr (kBytes >= 16) {
#pragma unroll
        for (int q = 0; q < kBytes / 16; q++) {
            const u32x4_g v = *(SKML_G(u32x4_g))(codes + b0 + 16 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    } else if constexpr (kBytes == 8) {
        const u32x2_g v = *(SKML_G(u32x2_g))(codes + b0);
        w[0] = v.x; w[1] = v.y;
    } else if constexpr (kBytes == 4) {
        w[0] = *(SKML_G(uint32_t))(codes + b0);
    } else if constexpr (kBytes == 2) {
        w[0] = *(SKML_G(uint16_t))(codes + b0);
    } else {
        w[0] = codes[b0];
    }
}
#undef SKML_G
template <int BITS, int PER = kOccPer>
__device__ __forceinline__ uint32_t code_occ_at(const uint32_t (&w)[occ_words<BITS, PER>()], int e) {
    return (w[(e * BITS) >> 5] >> ((e * BITS) & 31)) & ((1u << BITS) - 1u);
}

}  // namespace skml
