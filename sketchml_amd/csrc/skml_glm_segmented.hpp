// skml_glm_segmented.hpp -- the index arithmetic of the sparse mini-batch gradient's column sum in the
// segmented summation order (skml_glm_segmented.hip): how a column is classed by its length, the walk
// over a short column's entries by window membership (no search), which entries of a wide column a
// lane of a wave adds, how a very wide column is cut into slices, and the fixed butterfly that joins
// the 64 lane sums.  Everything is a function of a column's window count m and of the constants below,
// never of the device: that is what makes the order of every sum, and so its bits, the same on every
// run.  No device builtins: the kernels and the host program tests/glm_segmented_check.cpp
// instantiate the same functions.
#pragma once
#include <stdint.h>

#include "skml_glm.hpp"

namespace skml {

constexpr int kSegMSeq = 32;          // M_SEQ: a column of at most this many window entries is summed in batch order
constexpr int kSegSlice = 1024;       // window entries of one slice of a split column, a multiple of 64
constexpr int kSegSplitAt = 2 * kSegSlice;  // SPLIT_AT: window entries from which a column is cut into slices
constexpr int kSegV = 4;              // features a lane of the tile pass holds in flight
constexpr int kSegTile = 64 * kSegV;  // features of a wave's tile
constexpr int kSegE = 4;              // entries of a column the tile pass loads ahead of knowing its length
constexpr int kSegU = 8;              // entries a lane of the wide pass has in flight
static_assert(kSegSlice % 64 == 0, "p mod 64 names the same lane inside every slice");
static_assert(kSegSplitAt > kSegSlice && kSegSlice > kSegMSeq && kSegE <= kSegMSeq, "the classes nest");

// ---- classes of a column by its stored length ce - cs ----
constexpr int kSegEmpty = 0, kSegShort = 1, kSegLong = 2;
SKML_GLM_HD int seg_class(int64_t len) { return len <= 0 ? kSegEmpty : len <= kSegMSeq ? kSegShort : kSegLong; }

// A short column's sum: every stored entry is read and kept by comparison with the window, no search.
// The rows ascend, so the [0, b1) hits lie ahead of the [a0, a1) hits in memory; batch order is the
// second kind after the first, hence two walks.  With rows ascending this is glm_col_sum's order and
// bits; a batch position is inside [0, batch) by construction.
SKML_GLM_HD double seg_short_sum(const int32_t* csc_row, const double* csc_val, int64_t cs, int64_t ce, const GlmWindow& w,
                                 const double* coef) {
    const int64_t first = w.a1 - w.a0;
    double acc = 0.0;
    for (int64_t i = cs; i < ce; i++) {
        const int64_t j = (int64_t)csc_row[i] - w.a0;
        if ((uint64_t)j >= (uint64_t)first) continue;
        const double p = csc_val[i] * coef[j];
        acc += p;
    }
    if (w.b1 <= 0) return acc;
    for (int64_t i = cs; i < ce; i++) {
        const int64_t r = csc_row[i];
        if ((uint64_t)r >= (uint64_t)w.b1) continue;
        const double p = csc_val[i] * coef[first + r];
        acc += p;
    }
    return acc;
}

// ---- a wide column (more than kSegMSeq window entries): the work list's records ----
// The column's window entries in batch order are p = 0 .. m - 1: p < n0 is entry s0 + p of the [a0, a1)
// range, the others entry s1 + (p - n0) of the [0, b1) range.  unit0: the column's first unit; its slices
// take consecutive units, and a slice's partial sum has its unit's index.
struct SegItem {
    int64_t s0, s1;
    int32_t n0, m, k;
    uint32_t unit0;
};
struct SegUnit {
    int32_t item, slice;
};
// Both counts clamped so that they fit the record; n0 + n1 = m.  Ascending rows give m <= batch < 2^31.
SKML_GLM_HD SegItem seg_item(const GlmColRanges& r, int64_t k, uint32_t unit0) {
    const int64_t cap = 0x7FFFFFFFLL, a = r.e0 - r.s0, b = r.e1 - r.s1;
    const int64_t n0 = a < 0 ? 0 : (a > cap ? cap : a), n1 = b < 0 ? 0 : (b > cap - n0 ? cap - n0 : b);
    return SegItem{r.s0, r.s1, (int32_t)n0, (int32_t)(n0 + n1), (int32_t)k, unit0};
}
// NS(m): the slices, and so the units, of a column of m window entries.
SKML_GLM_HD int64_t seg_slices(int64_t m) { return m >= kSegSplitAt ? (m + kSegSlice - 1) / kSegSlice : 1; }
// The entries [*pb, *pe) of slice t of such a column; the whole column when it is not split.
SKML_GLM_HD void seg_slice_range(int64_t m, int64_t t, int64_t* pb, int64_t* pe) {
    if (m < kSegSplitAt) {
        *pb = 0;
        *pe = m;
        return;
    }
    *pb = t * kSegSlice;
    *pe = *pb + kSegSlice < m ? *pb + kSegSlice : m;
}
// Entry p's index in csc_row / csc_val, and the range it belongs to.
SKML_GLM_HD int64_t seg_entry_index(const SegItem& it, int64_t p, bool* second) {
    *second = p >= it.n0;
    return *second ? it.s1 + (p - it.n0) : it.s0 + p;
}
// Lane `lane`'s sum over [pb, pe): from +0.0 and in ascending p the entries with p mod 64 == lane (pb is a
// multiple of 64), kSegU of them loaded, gathered and multiplied ahead of their adds.  A slot past pe, or
// an entry whose batch position is out of range, adds +0.0, which changes no bit of a sum that began at
// +0.0 and only added.
SKML_GLM_HD double seg_lane_sum(const int32_t* csc_row, const double* csc_val, const SegItem& it, int64_t pb, int64_t pe,
                                int lane, const GlmWindow& w, const double* coef, int64_t batch) {
    double acc = 0.0;
    for (int64_t p0 = pb + lane; p0 < pe; p0 += (int64_t)64 * kSegU) {
        double prod[kSegU];
        for (int u = 0; u < kSegU; u++) {
            const int64_t p = p0 + (int64_t)u * 64;
            prod[u] = 0.0;
            if (p < pe) {
                bool second;
                const int64_t i = seg_entry_index(it, p, &second);
                const int64_t j = glm_batch_pos(w, csc_row[i], second);
                if ((uint64_t)j < (uint64_t)batch) prod[u] = csc_val[i] * coef[j];
            }
        }
        for (int u = 0; u < kSegU; u++) acc += prod[u];
    }
    return acc;
}
// The join of the 64 lane sums: at each distance 32, 16, 8, 4, 2, 1 every lane adds its partner's value
// to its own.  IEEE addition commutes, so both partners hold the same bits and lane 0's is the result.
SKML_GLM_HD double seg_butterfly(const double (&lane_sum)[64]) {
    double v[64], t[64];
    for (int l = 0; l < 64; l++) v[l] = lane_sum[l];
    for (int d = 32; d > 0; d >>= 1) {
        for (int l = 0; l < 64; l++) t[l] = v[l] + v[l ^ d];
        for (int l = 0; l < 64; l++) v[l] = t[l];
    }
    return v[0];
}

// ---- the work list's size, from the data set's shape alone ----
// A wide column stores more than kSegMSeq entries and columns share none, so there are at most
// nnz / (kSegMSeq + 1) of them and at most dim.  A column of m entries has at most m / kSegSlice + 1 units,
// so the units number at most the wide columns plus nnz / kSegSlice.
SKML_GLM_HD int64_t seg_item_cap(int64_t dim, int64_t nnz) {
    const int64_t c = nnz / (kSegMSeq + 1);
    return c < dim ? c : dim;
}
SKML_GLM_HD int64_t seg_unit_cap(int64_t dim, int64_t nnz) {
    const int64_t c = seg_item_cap(dim, nnz);
    return c ? c + nnz / kSegSlice : 0;
}
// Bytes of the staging: a head (the list counter and the overflow flag), the items, the units, and a
// partial sum per unit.
constexpr int64_t kSegHead = 256;
SKML_GLM_HD int64_t seg_stage_bytes(int64_t dim, int64_t nnz) {
    return kSegHead + seg_item_cap(dim, nnz) * (int64_t)sizeof(SegItem) + seg_unit_cap(dim, nnz) * (int64_t)(sizeof(SegUnit) + 8);
}

}  // namespace skml
