// sparse_lowp_check.cpp -- sketchml_amd/csrc/skml_lowp.hpp on the host, for every 16-bit pattern of
// bf16 and fp16: the widening equals the value its sign, exponent and mantissa fields spell out, and
// the 16-bit keep test equals the fp32 keep test of the widened value, which equals
// DenseDoubleGradient.toSparse's |x| > 1e-8 in double with NaN dropped and +-inf kept.
// Built with -fsanitize=address,undefined and run as a program of its own (tests/test_sparse_lowp_cpu.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../sketchml_amd/csrc/skml_lowp.hpp"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, sizeof f);
    return f;
}
static uint32_t to_bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, sizeof b);
    return b;
}

// The value of a pattern with E exponent bits and M mantissa bits (bias 2^(E-1) - 1), from its
// fields; false for a NaN.
template <int E, int M>
static bool field_value(uint16_t h, float* out) {
    const int bias = (1 << (E - 1)) - 1;
    const uint32_t s = h >> 15, e = (h >> M) & ((1u << E) - 1u), m = h & ((1u << M) - 1u);
    double v;
    if (e == (1u << E) - 1u) {
        if (m) return false;
        v = INFINITY;
    } else if (e == 0) {
        v = std::ldexp((double)m, 1 - bias - M);
    } else {
        v = std::ldexp((double)((1u << M) + m), (int)e - bias - M);
    }
    *out = (float)(s ? -v : v);  // exact: every bf16 / fp16 value is a float
    return true;
}

template <int E, int M>
static int check(const char* name, uint32_t (*widen)(uint16_t), bool (*keep)(uint16_t)) {
    int bad = 0;
    for (uint32_t i = 0; i < 65536; i++) {
        const uint16_t h = (uint16_t)i;
        const uint32_t wb = widen(h);
        const float w = from_bits(wb);
        float want = 0.0f;
        if (field_value<E, M>(h, &want)) {
            if (to_bits(want) != wb) {
                if (bad++ < 8) std::printf("%s 0x%04X widens to 0x%08X, its fields say 0x%08X\n", name, h, wb, to_bits(want));
            }
        } else {  // a NaN: sign kept, mantissa in the float's top mantissa bits
            const uint32_t nan = ((uint32_t)(h & 0x8000u) << 16) | 0x7F800000u | ((uint32_t)(h & ((1u << M) - 1u)) << (23 - M));
            if (!std::isnan(w) || wb != nan) {
                if (bad++ < 8) std::printf("%s NaN 0x%04X widens to 0x%08X, expected 0x%08X\n", name, h, wb, nan);
            }
        }
        const double d = (double)w;
        const bool ref = !std::isnan(d) && std::fabs(d) > 1e-8;
        if (keep(h) != ref || skml::keep_f32_bits(wb) != ref) {
            if (bad++ < 8)
                std::printf("%s 0x%04X (%a): keep %d, fp32 keep of the widened value %d, |x| > 1e-8 %d\n", name, h, d,
                            (int)keep(h), (int)skml::keep_f32_bits(wb), (int)ref);
        }
    }
    return bad;
}

int main() {
    int bad = 0;
    bad += check<8, 7>("bf16", skml::widen_bf16_bits, skml::keep_bf16_bits);
    bad += check<5, 10>("fp16", skml::widen_f16_bits, skml::keep_f16_bits);
    // the neighbours of the threshold named in the header's comment, and fp16's smallest subnormal
    if (skml::keep_bf16_bits(0x322B) || skml::keep_bf16_bits(0xB22B) || !skml::keep_bf16_bits(0x322C) ||
        !skml::keep_bf16_bits(0xB22C) || !skml::keep_f16_bits(0x0001) || !skml::keep_f16_bits(0x8001)) {
        std::printf("threshold neighbours\n");
        bad++;
    }
    if (bad) {
        std::printf("FAILED: %d\n", bad);
        return 1;
    }
    std::printf("ok 131072 patterns\n");
    return 0;
}
