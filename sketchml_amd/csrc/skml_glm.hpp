// skml_glm.hpp -- the index arithmetic of the mini-batch gradient (ml/objective/GradientDescent.scala:23-51):
// the looping window of DataSet.loopingRead (ml/data/DataSet.scala:15-21) as two row ranges, a column's
// entries inside each range by binary search, and the walk over them in batch order, which is
// DenseDoubleGradient.plusBy's addition order (DenseDoubleGradient.scala:51-57) seen from one feature.
// No device builtins: the kernels of skml_glm.hip and the host program tests/glm_check.cpp
// instantiate the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SKML_GLM_HD __host__ __device__ inline
#else
#define SKML_GLM_HD inline
#endif

namespace skml {

// The batch's rows in batch order: [a0, a1) first, then [0, b1).  b1 = 0 when the window does not wrap.
struct GlmWindow {
    int64_t a0, a1, b1;
};

// batch instances from row0 of a data set of `rows` (0 <= row0 < rows, 1 <= batch <= rows).
SKML_GLM_HD GlmWindow glm_window(int64_t rows, int64_t row0, int64_t batch) {
    const int64_t end = row0 + batch;
    return end <= rows ? GlmWindow{row0, end, 0} : GlmWindow{row0, rows, end - rows};
}

// The row of batch position j.
SKML_GLM_HD int64_t glm_row_of(const GlmWindow& w, int64_t j) {
    const int64_t first = w.a1 - w.a0;
    return j < first ? w.a0 + j : j - first;
}

// The first index in [lo, hi) of the ascending rows[] that holds a value >= r (hi when none does).
SKML_GLM_HD int64_t glm_lower_bound(const int32_t* rows, int64_t lo, int64_t hi, int64_t r) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)rows[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// A column's entries of the window: [s0, e0) belong to the rows [a0, a1), [s1, e1) to [0, b1).
struct GlmColRanges {
    int64_t s0, e0, s1, e1;
    SKML_GLM_HD int64_t count() const { return (e0 - s0) + (e1 - s1); }
};

// The entries [cs, ce) of one column, rows ascending in csc_row.
SKML_GLM_HD GlmColRanges glm_col_ranges(const int32_t* csc_row, int64_t cs, int64_t ce, const GlmWindow& w) {
    GlmColRanges r;
    r.s0 = glm_lower_bound(csc_row, cs, ce, w.a0);
    r.e0 = glm_lower_bound(csc_row, r.s0, ce, w.a1);
    r.s1 = cs;
    r.e1 = w.b1 > 0 ? glm_lower_bound(csc_row, cs, r.s0, w.b1) : cs;
    return r;
}

// The batch position of the entry at index i of the first (second = false) or second range; the
// caller refuses a position outside [0, batch), which only an unsorted csc_row can give.
SKML_GLM_HD int64_t glm_batch_pos(const GlmWindow& w, int64_t row, bool second) {
    return second ? (w.a1 - w.a0) + row : row - w.a0;
}

// g[k] of plusBy: from +0.0, val * coef[j] (rounded, then added) for the column's entries in batch
// order: the first range's, then the second's.
SKML_GLM_HD double glm_col_sum(const int32_t* csc_row, const double* csc_val, const GlmColRanges& r, const GlmWindow& w,
                               const double* coef, int64_t batch) {
    double acc = 0.0;
    for (int64_t i = r.s0; i < r.e0; i++) {
        const int64_t j = glm_batch_pos(w, csc_row[i], false);
        if ((uint64_t)j >= (uint64_t)batch) continue;
        const double p = csc_val[i] * coef[j];
        acc += p;
    }
    for (int64_t i = r.s1; i < r.e1; i++) {
        const int64_t j = glm_batch_pos(w, csc_row[i], true);
        if ((uint64_t)j >= (uint64_t)batch) continue;
        const double p = csc_val[i] * coef[j];
        acc += p;
    }
    return acc;
}

}  // namespace skml
