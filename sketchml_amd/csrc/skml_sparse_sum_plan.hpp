// skml_sparse_sum_plan.hpp -- how Gradient.sum (skml_sparse_blob.cpp, decode_sum_any) cuts its P
// payloads into scratch batches, shared with the host check tests/sum_plan_check.cpp.  Plain C++
// (no HIP types) so that the host compiler builds it alone.
#pragma once
#include <stddef.h>

#include <vector>

namespace skml {

// The scratch budget of one batch: the restored keys, bins and run bounds of its payloads.  The
// batch's key and bin offsets travel as int32 (AggPayload::gk_off / gb_off), which 3 GiB keeps
// below 2^31 words and bytes.
constexpr size_t kSumBudget = (size_t)3 << 30;

// Greedy batches in payload order: a batch takes payloads while the sum of their `need` bytes stays
// within `budget`, and always takes at least one (a payload above the budget forms a batch of its
// own).  Returns the batches' end indices: batch b holds payloads [ends[b - 1], ends[b]), ends[-1]
// read as 0; the last entry is need.size().  No sum of needs is formed that could wrap size_t.
inline std::vector<size_t> plan_sum_batches(const std::vector<size_t>& need, size_t budget) {
    std::vector<size_t> ends;
    size_t at = 0, bytes = 0;  // the open batch: its first payload and its bytes so far
    for (size_t p = 0; p < need.size(); p++) {
        // bytes + need[p] <= budget, without forming the sum
        const bool fits = bytes <= budget && need[p] <= budget - bytes;
        if (p > at && !fits) {  // p opens the next batch; a batch's first payload is never turned away
            ends.push_back(p);
            at = p;
            bytes = 0;
        }
        bytes += need[p];
    }
    if (!need.empty()) ends.push_back(need.size());
    return ends;
}

}  // namespace skml
