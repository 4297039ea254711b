// The in-register half-clean stages of a bitonic merge, two stages at a time in 3-input form.
//
// halfclean_paired<R, STAGES, Ops>(v) runs the stages d = R/2, R/4, ... (STAGES of them) of the
// half-cleaner over the cyclic-bitonic register sequence v[0..R), like the plain loop
//     for each stage d: for each i with (i & d) == 0: (v[i], v[i+d]) = (min, max)(v[i], v[i+d]).
// Two consecutive stages d and h = d/2 touch the registers in groups of four, a = v[i],
// b = v[i+h], c = v[i+d], e = v[i+d+h] ((i & d) == 0, (i & h) == 0).  The plain form takes 8 ops per
// group: lo = min(a,c), hi = max(a,c), lo' = min(b,e), hi' = max(b,e), then (lo, lo') and
// (hi, hi').  Here lo' and hi' are never computed (6 ops):
//     v[i]   = min(lo, lo')           = min3(b, e, lo)
//     v[i+h] = max(lo, min(b, e))     = med3(b, e, lo)    needs lo <= max(b, e)
//     v[i+d] = min(hi, max(b, e))     = med3(b, e, hi)    needs hi >= min(b, e)
//     v[i+d+h] = max(hi, hi')         = max3(b, e, hi)
// Both conditions hold for any four equally spaced elements of a cyclic-bitonic sequence, and every
// sub-sequence a half-cleaner leaves is bitonic again, so the form applies at every stage pair
// (tests/halfclean_check.cpp: every 0-1 cyclic-bitonic input for R = 4..64, by the 0-1 principle,
// and random floats).  An odd STAGES leaves the last stage in the plain form.
//
// Ops supplies min2 / max2 / min3 / med3 / max3 over T, fence() (a scheduling barrier, or nothing)
// and kFenceGroups (groups of four between fences, 0 = none).  No device builtin appears here, so
// a host compiler builds the same template with a host policy.
#pragma once

#if defined(__HIPCC__)
#define SKML_HC_FN __device__ __forceinline__
#define SKML_HC_UNROLL _Pragma("unroll")
#else
#define SKML_HC_FN inline
#define SKML_HC_UNROLL
#endif

constexpr int halfclean_log2(int r) { return r <= 1 ? 0 : 1 + halfclean_log2(r / 2); }

// The stages from distance D down, STAGES of them.
template <int R, int D, int STAGES, typename Ops, typename T>
SKML_HC_FN void halfclean_paired_from(T (&v)[R]) {
    if constexpr (STAGES >= 2) {
        constexpr int H = D / 2;
        static_assert(H >= 1, "more stages than the registers have");
        SKML_HC_UNROLL
        for (int i = 0; i < R; i++) {
            if ((i & D) != 0 || (i & H) != 0) continue;
            const T b = v[i + H], e = v[i + D + H];
            const T lo = Ops::min2(v[i], v[i + D]);
            const T hi = Ops::max2(v[i], v[i + D]);
            v[i] = Ops::min3(b, e, lo);
            v[i + H] = Ops::med3(b, e, lo);
            v[i + D] = Ops::med3(b, e, hi);
            v[i + D + H] = Ops::max3(b, e, hi);
            if constexpr (Ops::kFenceGroups > 0) {
                // i counts 4 registers per group within a block of 2 D
                const int g = (i / (2 * D)) * H + (i & (H - 1));
                if (g % Ops::kFenceGroups == Ops::kFenceGroups - 1) Ops::fence();
            }
        }
        halfclean_paired_from<R, D / 4, STAGES - 2, Ops>(v);
    } else if constexpr (STAGES == 1) {
        static_assert(D >= 1, "more stages than the registers have");
        SKML_HC_UNROLL
        for (int i = 0; i < R; i++) {
            if ((i & D) != 0) continue;
            const T lo = Ops::min2(v[i], v[i + D]);
            const T hi = Ops::max2(v[i], v[i + D]);
            v[i] = lo;
            v[i + D] = hi;
        }
    }
}

template <int R, int STAGES, typename Ops, typename T>
SKML_HC_FN void halfclean_paired(T (&v)[R]) {
    static_assert(R >= 2 && (R & (R - 1)) == 0, "R is a power of two");
    static_assert(STAGES >= 0 && STAGES <= halfclean_log2(R), "at most log2 R stages");
    halfclean_paired_from<R, R / 2, STAGES, Ops>(v);
}
