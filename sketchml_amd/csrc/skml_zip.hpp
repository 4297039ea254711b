// skml_zip.hpp -- index arithmetic of the ZipMLQuantizer split search (ml/gradient/ZipGradient.scala:
// 85-115) shared by the kernels of skml_zip.hip and by the host check tests/zip_check.cpp: the
// order-preserving keys, a pair's error operands and error, the select's digit walk and the
// compaction's output offsets.  Plain C++ (no HIP types) so that the host compiler builds it too.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SKML_ZIP_HD __host__ __device__ inline
#else
#define SKML_ZIP_HD inline
#endif

namespace skml {

// Arrays.sort(double[])'s total order as an unsigned order: all bits of a negative flipped, the
// sign bit of a non-negative flipped (-0.0 before +0.0, NaN above +inf / below -inf).
SKML_ZIP_HD uint64_t zip_key64(double d) {
    const uint64_t b = __builtin_bit_cast(uint64_t, d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
SKML_ZIP_HD double zip_unkey64(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
    return __builtin_bit_cast(double, b);
}
SKML_ZIP_HD uint32_t zip_key32(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
SKML_ZIP_HD float zip_unkey32(uint32_t k) {
    const uint32_t b = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
    return __builtin_bit_cast(float, b);
}
// A key of a NaN or an infinity (exponent all ones).
SKML_ZIP_HD bool zip_bad64(double d) {
    return (__builtin_bit_cast(uint64_t, d) & 0x7FF0000000000000ULL) == 0x7FF0000000000000ULL;
}
SKML_ZIP_HD bool zip_bad32(float f) { return (__builtin_bit_cast(uint32_t, f) & 0x7F800000u) == 0x7F800000u; }

constexpr int kZipDigitBits = 8;
constexpr int kZipDigits = 1 << kZipDigitBits;
// Digit `pass` (0 = least significant) of a key.
SKML_ZIP_HD int zip_digit(uint64_t key, int pass) { return (int)((key >> (kZipDigitBits * pass)) & (kZipDigits - 1)); }

// The sort passes' shape: a workgroup of kZsThreads scatters its tile of kZsTile keys in steps of
// kZsRows rows of kZsThreads keys, a thread one key of each row.
constexpr int kZsThreads = 256;
constexpr int kZsWaves = kZsThreads / 64;
constexpr int kZsTile = kZsThreads * 32;  // keys per workgroup of a sort pass
constexpr int kZsRows = 4;

// splitIndex[j] of a round; idx == nullptr is round 1's identity.
SKML_ZIP_HD int64_t zip_split_at(const int32_t* idx, int64_t j) { return idx ? (int64_t)idx[j] : j; }

// Pair i of a round over split_num splits of n sorted values: the value range [L, R] it covers
// (ZipGradient.scala:90-91).
SKML_ZIP_HD void zip_pair_range(const int32_t* idx, int64_t i, int64_t split_num, int64_t n, int64_t* L, int64_t* R) {
    *L = zip_split_at(idx, 2 * i);
    *R = (2 * i + 2 >= split_num ? n : zip_split_at(idx, 2 * i + 2)) - 1;
}

// errors(i) of ZipGradient.scala:92-95 from the prefix sums r, t: this association, in double,
// built without contraction.
SKML_ZIP_HD double zip_pair_error(const double* r, const double* t, int64_t L, int64_t R) {
    const double l1 = r[R] - (L == 0 ? 0.0 : r[L - 1]);
    const double l2 = t[R] - (L == 0 ? 0.0 : t[L - 1]);
    const double cnt = (double)(R - L + 1);
    const double mean = l1 / cnt;
    return (l2 + (mean * mean) * cnt) - ((2.0 * mean) * l1);
}

// thrNum of a round (ZipGradient.scala:98).
SKML_ZIP_HD int64_t zip_thr_num(int64_t split_num, int bins) { return bins / 2 - (split_num & 1); }

// One step of the radix select for the k-th largest (k >= 1) key: hist[d] counts the candidates
// (keys equal to the digits already fixed) whose current digit is d.  Walks from the largest
// digit down; returns the digit holding the k-th largest and lowers *k to its rank inside it.
SKML_ZIP_HD int zip_select_digit(const uint32_t* hist, int64_t* k) {
    int64_t left = *k;
    for (int d = kZipDigits - 1; d > 0; d--) {
        if ((int64_t)hist[d] >= left) {
            *k = left;
            return d;
        }
        left -= hist[d];
    }
    *k = left;
    return 0;
}

// Output position of pair i's first split after the compaction: every pair before it wrote one
// split plus one more when it was kept; kept_before = exclusive scan of the keep flags.
SKML_ZIP_HD int64_t zip_out_pos(int64_t i, int64_t kept_before) { return i + kept_before; }

// Longest chain of additions behind one output of the prefix-sum tree of skml_zip.hip over n
// leaves of depth d0 (DESIGN.md "ZipML"): kZipScanItems - 1 inside a thread, 6 in the wave scan,
// 2 for the offset of the last of the 4 waves (3 for the workgroup total), one for wave offset +
// lane offset and one for the thread's own prefix; with more than one workgroup, the workgroup
// offset (out of the same tree over the workgroup totals) is added to wave + lane offset first, one
// addition more on either path.
constexpr int kZipScanThreads = 256;
constexpr int kZipScanItems = 8;
constexpr int kZipScanBlock = kZipScanThreads * kZipScanItems;  // 2,048 values per workgroup
SKML_ZIP_HD int zip_scan_depth(int64_t n, int d0) {
    const int local = d0 + (kZipScanItems - 1) + 6 + 2 + 1 + 1;
    if (n <= kZipScanBlock) return local;
    const int64_t nb = (n + kZipScanBlock - 1) / kZipScanBlock;
    const int up = zip_scan_depth(nb, d0 + (kZipScanItems - 1) + 6 + 3);
    return up + 2 > local + 1 ? up + 2 : local + 1;
}

}  // namespace skml
