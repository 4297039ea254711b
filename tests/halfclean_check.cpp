// Host check of the paired half-clean form (sketchml_amd/csrc/skml_halfclean.hpp, the template the
// leaf kernels instantiate) against the plain stages, for R = 4, 8, 16, 32, 64 and both stage counts
// in use (log2 R: halfclean_regs; log2 R - 1: halfclean_regs_compact_sel before its final med3):
//  - every 0-1 cyclic-bitonic input (R (R - 1) + 2 of them; every op is monotone, so by the 0-1
//    principle these decide every input);
//  - random float cyclic-bitonic inputs with duplicates, +-inf and equal runs, compared bit for bit.
// Prints "ok" and the number of inputs, or the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../sketchml_amd/csrc/skml_halfclean.hpp"

template <typename T>
struct HostOps {
    static constexpr int kFenceGroups = 2;  // the fence index arithmetic runs here too
    static inline long fences = 0;
    static T min2(T a, T b) { return b < a ? b : a; }
    static T max2(T a, T b) { return b < a ? a : b; }
    static T min3(T a, T b, T c) { return min2(min2(a, b), c); }
    static T max3(T a, T b, T c) { return max2(max2(a, b), c); }
    static T med3(T a, T b, T c) { return max2(min2(a, b), min2(max2(a, b), c)); }
    static void fence() { fences++; }
};

template <int R, int STAGES, typename T>
static void plain(T (&v)[R]) {
    int d = R / 2;
    for (int s = 0; s < STAGES; s++, d /= 2)
        for (int i = 0; i < R; i++)
            if ((i & d) == 0) {
                const T lo = HostOps<T>::min2(v[i], v[i + d]), hi = HostOps<T>::max2(v[i], v[i + d]);
                v[i] = lo;
                v[i + d] = hi;
            }
}

static long g_inputs = 0;

template <int R, int STAGES, typename T>
static bool same(const T (&in)[R], const char* what) {
    T a[R], b[R];
    std::memcpy(a, in, sizeof a);
    std::memcpy(b, in, sizeof b);
    plain<R, STAGES>(a);
    halfclean_paired<R, STAGES, HostOps<T>>(b);
    g_inputs++;
    if (std::memcmp(a, b, sizeof a) == 0) return true;
    std::printf("mismatch: R=%d stages=%d %s\n  in   ", R, STAGES, what);
    for (int i = 0; i < R; i++) std::printf(" %g", (double)in[i]);
    std::printf("\n  plain");
    for (int i = 0; i < R; i++) std::printf(" %g", (double)a[i]);
    std::printf("\n  pair ");
    for (int i = 0; i < R; i++) std::printf(" %g", (double)b[i]);
    std::printf("\n");
    return false;
}

// all 0-1 sequences with at most two cyclic transitions: `ones` ones starting at `rot`
template <int R, int STAGES>
static bool zero_one() {
    int v[R];
    long count = 0;
    for (int ones = 0; ones <= R; ones++) {
        const int rots = (ones == 0 || ones == R) ? 1 : R;
        for (int rot = 0; rot < rots; rot++) {
            for (int i = 0; i < R; i++) v[i] = ((i - rot + R) % R) < ones ? 1 : 0;
            if (!same<R, STAGES>(v, "0-1")) return false;
            count++;
        }
    }
    if (count != (long)R * (R - 1) + 2) {
        std::printf("R=%d: %ld 0-1 inputs, expected %ld\n", R, count, (long)R * (R - 1) + 2);
        return false;
    }
    // the full stage count sorts a bitonic sequence: a check of the plain restatement itself
    if (STAGES == halfclean_log2(R)) {
        for (int i = 0; i < R; i++) v[i] = (i % R) < R / 3 ? 1 : 0;
        halfclean_paired<R, STAGES, HostOps<int>>(v);
        for (int i = 1; i < R; i++)
            if (v[i - 1] > v[i]) {
                std::printf("R=%d: the full half-cleaner left the sequence unsorted\n", R);
                return false;
            }
    }
    return true;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 24);
}

// a rise of `up` values then a fall, drawn from a pool of `pool` values (small pool: duplicates and
// equal runs), some pushed to +-inf, rotated by `rot`
template <int R, int STAGES>
static bool random_floats(int trials) {
    const float inf = std::numeric_limits<float>::infinity();
    for (int t = 0; t < trials; t++) {
        const int pool = 1 + (int)(rnd() % (t % 3 == 0 ? 3 : (t % 3 == 1 ? R : 100000)));
        float s[R];
        for (int i = 0; i < R; i++) {
            const uint32_t k = rnd() % (uint32_t)pool, m = rnd() % 16;
            s[i] = m == 0 ? -inf : (m == 1 ? inf : ((float)k - 0.5f * (float)pool) * 0.37f + 0.001f);
        }
        const int up = (int)(rnd() % (R + 1)), rot = (int)(rnd() % R);
        // insertion sorts: ascending head, descending tail
        for (int i = 1; i < up; i++)
            for (int j = i; j > 0 && s[j] < s[j - 1]; j--) { const float x = s[j]; s[j] = s[j - 1]; s[j - 1] = x; }
        for (int i = up + 1; i < R; i++)
            for (int j = i; j > up && s[j] > s[j - 1]; j--) { const float x = s[j]; s[j] = s[j - 1]; s[j - 1] = x; }
        float v[R];
        for (int i = 0; i < R; i++) v[(i + rot) % R] = s[i];
        if (!same<R, STAGES>(v, "float")) return false;
    }
    return true;
}

template <int R>
static bool all_for() {
    constexpr int L = halfclean_log2(R);
    return zero_one<R, L>() && zero_one<R, L - 1>() && random_floats<R, L>(20000) && random_floats<R, L - 1>(20000);
}

int main() {
    const bool ok = all_for<4>() && all_for<8>() && all_for<16>() && all_for<32>() && all_for<64>();
    if (!ok) return 1;
    if (HostOps<int>::fences == 0 || HostOps<float>::fences == 0) {
        std::printf("no fence was placed\n");
        return 1;
    }
    std::printf("ok %ld\n", g_inputs);
    return 0;
}
