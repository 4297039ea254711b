// skml_valid.hpp -- the index arithmetic of the validation pass (ml/util/ValidationUtil.scala:12-93)
// shared by the kernels of skml_glm.hip / skml_valid.hip and the host program tests/valid_check.cpp:
// the classification of one instance, the chunk walk of the ordered sum, and the offsets of the
// stable key-and-payload scatter.  Plain C++ (no HIP types) so that the host compiler builds it too.
#pragma once
#include <stdint.h>

#include "skml_zip.hpp"

namespace skml {

// ValidationUtil.scala:23-29 for one instance.  z = pre * label is one rounded product; z == 0 (an
// underflow, a zero label, an empty row) and a NaN z move no counter.
enum : int { kValidNone = 0, kValidTruePos = 1, kValidTrueNeg = 2, kValidFalsePos = 3, kValidFalseNeg = 4 };
SKML_ZIP_HD int valid_class(double pre, double label) {
    const double z = pre * label;
    if (z > 0) return pre > 0 ? kValidTruePos : kValidTrueNeg;
    if (z < 0) return pre > 0 ? kValidFalsePos : kValidFalseNeg;
    return kValidNone;
}

// The ordered sum walks x[0 .. n) in steps of kSeqStep values, kSeqU chunks of 64 (a lane one value of
// each chunk).  seq_chunk_count: how many values of chunk u of the step at b exist (0 .. 64).
constexpr int kSeqU = 4;
constexpr int kSeqStep = kSeqU * 64;
SKML_ZIP_HD int64_t seq_index(int64_t b, int u, int lane) { return b + (int64_t)u * 64 + lane; }
SKML_ZIP_HD int seq_chunk_count(int64_t n, int64_t b, int u) {
    const int64_t rem = n - (b + (int64_t)u * 64);
    return rem <= 0 ? 0 : (rem < 64 ? (int)rem : 64);
}

// The scatter of one sort pass (k_zip_scatter's scheme): workgroup `block` owns the keys [b0, e) of its
// tile and moves them in steps of kZsRows rows of kZsThreads keys.  Key (row j, thread tid) of the step
// at s0 is input position s0 + j * kZsThreads + tid; its (row, wave) slot is j * kZsWaves + tid / 64.
constexpr int kValidSlots = kZsRows * kZsWaves;
SKML_ZIP_HD void valid_tile(int64_t block, int64_t n, int64_t* b0, int64_t* e) {
    *b0 = block * (int64_t)kZsTile;
    *e = *b0 + kZsTile < n ? *b0 + kZsTile : n;
}
SKML_ZIP_HD int64_t valid_step_index(int64_t s0, int row, int tid) { return s0 + (int64_t)row * kZsThreads + tid; }
SKML_ZIP_HD int valid_slot(int row, int wave) { return row * kZsWaves + wave; }
// One digit's counts of the step's slots (cnt[q * stride]) become the slots' first output positions
// (off[q * stride]) in (row, wave) order from `base` on; the counts are cleared for the next step.
// Returns the digit's base after the step.
SKML_ZIP_HD uint32_t valid_slot_offsets(uint32_t base, uint32_t* cnt, uint32_t* off, int stride) {
    uint32_t run = base;
    for (int q = 0; q < kValidSlots; q++) {
        const uint32_t c = cnt[q * stride];
        off[q * stride] = run;
        cnt[q * stride] = 0u;
        run += c;
    }
    return run;
}

}  // namespace skml
