// glm_segmented_check.cpp -- sketchml_amd/csrc/skml_glm_segmented.hpp on the host, for one column of each window
// count around the order's constants over a window that wraps: every entry visited once, the short walk's bits,
// the slices' cover, the work list's bound.  Built and run by tests/test_glm_segmented_cpu.py; prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sketchml_amd/csrc/skml_glm_segmented.hpp"

using namespace skml;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 17;
}
static double value() { return ((double)(next() % 2000001) / 1000000.0 - 1.0) * (double)(1ull << (next() % 41)) / 1048576.0; }

// One column of m window entries and `outside` stored entries between the window's two row ranges.
static int check(int64_t m, int64_t outside) {
    const int64_t wrapped = m / 3, rows = m + outside + 2, row0 = rows - (m - wrapped), batch = m ? m : 1;
    const GlmWindow w = glm_window(rows, m ? row0 : rows - 1, batch);
    std::vector<int32_t> row;
    for (int64_t r = 0; r < wrapped; r++) row.push_back((int32_t)r);
    for (int64_t r = 0; r < outside; r++) row.push_back((int32_t)(wrapped + 1 + r));
    for (int64_t r = row0; m && r < rows; r++) row.push_back((int32_t)r);
    const int64_t len = (int64_t)row.size();
    std::vector<double> val((size_t)len), coef((size_t)batch);
    for (double& v : val) v = value();
    for (double& v : coef) v = value();
    const GlmColRanges r = glm_col_ranges(row.data(), 0, len, w);
    if (r.count() != m) return std::printf("m=%lld: the window holds %lld\n", (long long)m, (long long)r.count());
    const double seq = glm_col_sum(row.data(), val.data(), r, w, coef.data(), batch);
    const double got = seg_class(len) == kSegShort ? seg_short_sum(row.data(), val.data(), 0, len, w, coef.data()) : seq;
    if (std::memcmp(&got, &seq, 8)) return std::printf("m=%lld: the short walk gives %a, glm_col_sum %a\n", (long long)m, got, seq);
    const SegItem it = seg_item(r, 7, 0);
    const int64_t ns = seg_slices(m);
    if (it.m != m || ns * kSegSlice < m * (ns > 1) || (ns > 1 && (ns - 1) * kSegSlice >= m) || (ns > 1) != (m >= kSegSplitAt))
        return std::printf("m=%lld: %lld slices\n", (long long)m, (long long)ns);
    // every entry once, each by the lane p mod 64, in ascending p; the order's sum against its definition
    std::vector<int> seen((size_t)len, 0);
    double total = 0.0, mag = 0.0;
    for (int64_t t = 0; t < ns; t++) {
        int64_t pb, pe;
        seg_slice_range(m, t, &pb, &pe);
        double lanes[64], want[64] = {};
        for (int64_t p = pb; p < pe; p++) {
            bool second;
            const int64_t i = seg_entry_index(it, p, &second);
            if (i < 0 || i >= len) return std::printf("m=%lld: entry %lld at %lld\n", (long long)m, (long long)p, (long long)i);
            seen[(size_t)i]++;
            const double prod = val[(size_t)i] * coef[(size_t)glm_batch_pos(w, row[(size_t)i], second)];
            want[p % 64] += prod;
            mag += prod < 0 ? -prod : prod;
        }
        for (int l = 0; l < 64; l++) {
            lanes[l] = seg_lane_sum(row.data(), val.data(), it, pb, pe, l, w, coef.data(), batch);
            if (std::memcmp(&lanes[l], &want[l], 8)) return std::printf("m=%lld: lane %d of slice %lld\n", (long long)m, l, (long long)t);
        }
        const double s = seg_butterfly(lanes);
        total = ns > 1 ? total + s : s;
    }
    for (int64_t i = 0; i < len; i++) {
        const bool in = (i >= r.s0 && i < r.e0) || (i >= r.s1 && i < r.e1);
        if (seen[(size_t)i] != (in ? 1 : 0)) return std::printf("m=%lld: entry %lld visited %d times\n", (long long)m, (long long)i, seen[(size_t)i]);
    }
    const double tol = 2.0 * (double)m * 0x1p-53 * mag;  // two sums of m rounded terms, each within gamma_m of the exact one
    if (!(total - seq <= tol && seq - total <= tol) || (m <= 1 && std::memcmp(&total, &seq, 8))) return std::printf("m=%lld: %a against %a\n", (long long)m, total, seq);
    // the work list's bound for a data set of this one column, alone or among empty ones
    const int64_t wide = m > kSegMSeq ? 1 : 0;
    for (int64_t dim : {(int64_t)1, (int64_t)1000})
        if (wide > seg_item_cap(dim, len) || wide * ns > seg_unit_cap(dim, len)) return std::printf("m=%lld: the list's bound\n", (long long)m);
    return 0;
}

int main() {
    const int64_t counts[] = {0, 1, kSegMSeq - 1, kSegMSeq, kSegMSeq + 1, 63, 64, 65, 129, kSegSplitAt - 1, kSegSplitAt,
                              kSegSplitAt + 1, kSegSlice + 1, 3 * kSegSlice + 5};
    for (int64_t m : counts)
        for (int64_t outside : {(int64_t)0, (int64_t)3, (int64_t)kSegMSeq + 5})
            if (check(m, outside)) return 1;
    std::printf("ok\n");
    return 0;
}
