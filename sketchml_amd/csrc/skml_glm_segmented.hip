// skml_glm_segmented.hip -- the sparse mini-batch gradient's column sum in the segmented summation order
// (skml_glm_gradient_segmented_*; the order and its index arithmetic are skml_glm_segmented.hpp's):
//   k_glm_seg_tiles   a wave owns kSegTile consecutive features, kSegV per lane.  col_ptr is read coalesced
//                     for the whole tile before anything depends on it, then the first kSegE rows of every
//                     column, then their values and coefficients: three rounds of independent loads where
//                     k_glm_plus_by walks col_ptr -> three searches -> row -> value per lane.  A column of
//                     at most kSegMSeq window entries is summed by its lane in batch order (the sequential
//                     entry's bits); a wider one goes to the work list in the context's staging.
//   k_glm_seg_wide    a persistent grid over the work list's units: a wave per column, or per slice of a
//                     split column; lane l adds the entries p = l mod 64 with kSegU in flight, a butterfly
//                     joins the lanes.  An unsplit column's sum is g[k]; a slice's goes to staging.
//   k_glm_seg_reduce  a lane per split column adds its slices' partial sums in slice order.
// No floating-point atomic: the list counter is the only atomic, an integer, and the list's order enters
// no sum.  Every sum starts at +0.0 and only adds, so it never holds -0.0 and an added +0.0 changes no bit.
#include <algorithm>

#include "skml_device.hpp"
#include "skml_glm.hpp"
#include "skml_glm_segmented.hpp"
#include "skml_opt.hpp"

namespace skml {

namespace {

__device__ __forceinline__ int64_t seg_clamp(int64_t p, int64_t nnz) { return p < 0 ? 0 : (p > nnz ? nnz : p); }
__device__ __forceinline__ int64_t seg_lane_i64(int64_t x, int src) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)x, src);
    const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)x >> 32), src);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

}  // namespace

// The staging's head: the list counter (items in the low word, units in the high one: a wave reserves both
// with one atomic) and the flag of a reservation that did not fit, after which the list is not walked.
struct SegHead {
    unsigned long long list;
    unsigned int overflow;
};
static_assert(sizeof(SegHead) <= kSegHead, "the head's room in the staging");

__global__ __launch_bounds__(256) void k_glm_seg_tiles(skml_glm_data d, GlmWindow win, int64_t batch,
                                                       const double* __restrict__ coef, double* __restrict__ g,
                                                       SegHead* head, SegItem* __restrict__ items,
                                                       SegUnit* __restrict__ units, int64_t item_cap, int64_t unit_cap,
                                                       unsigned long long* count) {
    __shared__ unsigned long long s_cnt;
    const int lane = threadIdx.x & 63;
    const int64_t first = win.a1 - win.a0;
    const int64_t tiles = (d.dim + kSegTile - 1) / kSegTile;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
    LiveCount lc;
    // the trip count is the wave's: the cross-lane reads and the ballots need every lane
    for (int64_t tile = wave; tile < tiles; tile += waves) {
        const int64_t base = tile * kSegTile;
        // round 1: the tile's column pointers, feature base + v * 64 + lane in slot v
        int64_t cs[kSegV], ce[kSegV];
#pragma unroll
        for (int v = 0; v < kSegV; v++) cs[v] = seg_clamp(d.col_ptr[std::min<int64_t>(base + v * 64 + lane, d.dim)], d.nnz);
        const int64_t after = seg_clamp(d.col_ptr[std::min<int64_t>(base + kSegTile, d.dim)], d.nnz);
#pragma unroll
        for (int v = 0; v < kSegV; v++) {
            const int64_t next = __shfl_down(cs[v], 1);
            const int64_t wrap = v + 1 < kSegV ? seg_lane_i64(cs[v + 1], 0) : after;
            ce[v] = lane == 63 ? wrap : next;
            if (base + v * 64 + lane >= d.dim || ce[v] < cs[v]) ce[v] = cs[v];
        }
        // round 2: the first rows of every column, whatever its length turns out to be
        int32_t row[kSegV][kSegE];
#pragma unroll
        for (int v = 0; v < kSegV; v++)
#pragma unroll
            for (int e = 0; e < kSegE; e++) row[v][e] = cs[v] + e < ce[v] ? d.csc_row[cs[v] + e] : -1;
        // round 3: window membership by comparison, then the values and the coefficients of the hits
        double prod[kSegV][kSegE];
        unsigned in_first[kSegV];
#pragma unroll
        for (int v = 0; v < kSegV; v++) {
            in_first[v] = 0;
#pragma unroll
            for (int e = 0; e < kSegE; e++) {
                const int64_t r = row[v][e], j0 = r - win.a0;
                const bool h0 = r >= 0 && (uint64_t)j0 < (uint64_t)first, h1 = r >= 0 && r < win.b1;
                prod[v][e] = 0.0;
                if (h0 || h1) prod[v][e] = d.csc_val[cs[v] + e] * coef[h0 ? j0 : first + r];
                in_first[v] |= (unsigned)h0 << e;
            }
        }
        // the sums: a column of at most kSegE entries from the registers, the rest by its class
#pragma unroll
        for (int v = 0; v < kSegV; v++) {
            const int64_t k = base + v * 64 + lane, len = ce[v] - cs[v];
            const bool on = k < d.dim;
            double acc = 0.0;
            GlmColRanges r{0, 0, 0, 0};
            bool wide = false;
            if (len <= kSegE) {
                // the [a0, a1) hits in stored order, then the [0, b1) hits: a slot of the other kind adds +0.0
#pragma unroll
                for (int e = 0; e < kSegE; e++) acc += ((in_first[v] >> e) & 1) ? prod[v][e] : 0.0;
#pragma unroll
                for (int e = 0; e < kSegE; e++) acc += ((in_first[v] >> e) & 1) ? 0.0 : prod[v][e];
            } else if (seg_class(len) == kSegShort) {
                acc = seg_short_sum(d.csc_row, d.csc_val, cs[v], ce[v], win, coef);
            } else {
                r = glm_col_ranges(d.csc_row, cs[v], ce[v], win);
                if (r.count() <= kSegMSeq) acc = glm_col_sum(d.csc_row, d.csc_val, r, win, coef, batch);
                else wide = true;
            }
            // the wide columns of this slot: their place in the list from a ballot prefix and one atomic
            const unsigned long long mask = __ballot(wide);
            if (mask) {
                const SegItem mine = seg_item(r, k, 0);
                const int my_units = wide ? (int)seg_slices(mine.m) : 0;
                unsigned before = 0, total = 0;
                for (unsigned long long mm = mask; mm; mm &= mm - 1) {
                    const int src = __ffsll((long long)mm) - 1;
                    const unsigned n = (unsigned)__builtin_amdgcn_readlane(my_units, src);
                    if (src < lane) before += n;
                    total += n;
                }
                const unsigned cols = (unsigned)__popcll(mask);
                unsigned long long at = 0;
                if (lane == 0) at = atomicAdd(&head->list, ((unsigned long long)total << 32) | cols);
                at = (unsigned long long)seg_lane_i64((int64_t)at, 0);
                const uint64_t item0 = at & 0xFFFFFFFFull, unit0 = at >> 32;
                const bool fits = item0 + cols <= (uint64_t)item_cap && unit0 + total <= (uint64_t)unit_cap;
                if (!fits) {
                    if (lane == 0) head->overflow = 1;
                } else if (wide) {
                    const uint64_t it = item0 + (uint64_t)__popcll(mask & ((1ull << lane) - 1));
                    SegItem rec = mine;
                    rec.unit0 = (uint32_t)(unit0 + before);
                    items[it] = rec;
                    for (int t = 0; t < my_units; t++) units[rec.unit0 + t] = SegUnit{(int32_t)it, t};
                }
            }
            if (on && !wide) g[k] = acc;
            lc.add(on && !wide && fabs(acc) > 1e-8);  // DenseDoubleGradient.countNNZ; the wide columns are counted where they are summed
        }
    }
    lc.finish(&s_cnt, count);
}

__global__ __launch_bounds__(256) void k_glm_seg_wide(skml_glm_data d, GlmWindow win, int64_t batch,
                                                      const double* __restrict__ coef, double* __restrict__ g,
                                                      const SegHead* head, const SegItem* __restrict__ items,
                                                      const SegUnit* __restrict__ units, double* __restrict__ partial,
                                                      unsigned long long* count) {
    __shared__ unsigned long long s_cnt;
    if (head->overflow) return;  // the whole grid: the list is not to be trusted
    const int lane = threadIdx.x & 63;
    const int64_t n_units = (int64_t)(head->list >> 32);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
    LiveCount lc;
    for (int64_t u = wave; u < n_units; u += waves) {  // wave-uniform
        const SegUnit un = units[u];
        const SegItem it = items[un.item];
        int64_t pb, pe;
        seg_slice_range(it.m, un.slice, &pb, &pe);
        double a = seg_lane_sum(d.csc_row, d.csc_val, it, pb, pe, lane, win, coef, batch);
#pragma unroll
        for (int dist = 32; dist > 0; dist >>= 1) a += __shfl_xor(a, dist);
        const bool whole = seg_slices(it.m) == 1;
        if (lane == 0) {
            if (whole) g[it.k] = a;
            else partial[u] = a;
        }
        lc.add(whole && lane == 0 && fabs(a) > 1e-8);
    }
    lc.finish(&s_cnt, count);
}

__global__ __launch_bounds__(256) void k_glm_seg_reduce(double* __restrict__ g, const SegHead* head,
                                                        const SegItem* __restrict__ items,
                                                        const double* __restrict__ partial, unsigned long long* count) {
    __shared__ unsigned long long s_cnt;
    if (head->overflow) return;
    const int64_t n_items = (int64_t)(head->list & 0xFFFFFFFFull);
    const int lane = threadIdx.x & 63;
    LiveCount lc;
    for (int64_t b = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); b < n_items; b += (int64_t)gridDim.x * 256) {
        const int64_t c = b + lane;
        bool live = false;
        if (c < n_items) {
            const SegItem it = items[c];
            const int64_t ns = seg_slices(it.m);
            if (ns > 1) {
                double acc = 0.0;
                for (int64_t t = 0; t < ns; t++) acc += partial[(int64_t)it.unit0 + t];
                g[it.k] = acc;
                live = fabs(acc) > 1e-8;
            }
        }
        lc.add(live);
    }
    lc.finish(&s_cnt, count);
}

// stage: seg_stage_bytes(d.dim, d.nnz) bytes of the context's staging, ordered on st.
hipError_t launch_glm_segmented_plus_by(hipStream_t st, const skml_glm_data& d, int64_t row0, int64_t batch, const double* coef,
                                        void* stage, double* g, unsigned long long* count) {
    if (batch < 1 || batch > d.rows || row0 < 0 || row0 >= d.rows || d.dim < 1 || !stage) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    const int64_t item_cap = seg_item_cap(d.dim, d.nnz), unit_cap = seg_unit_cap(d.dim, d.nnz);
    char* base = static_cast<char*>(stage);
    SegHead* head = reinterpret_cast<SegHead*>(base);
    SegItem* items = reinterpret_cast<SegItem*>(base + kSegHead);
    SegUnit* units = reinterpret_cast<SegUnit*>(base + kSegHead + item_cap * (int64_t)sizeof(SegItem));
    double* partial = reinterpret_cast<double*>(base + kSegHead + item_cap * (int64_t)sizeof(SegItem) + unit_cap * (int64_t)sizeof(SegUnit));
    hipError_t e = hipMemsetAsync(head, 0, sizeof(SegHead), st);
    if (e != hipSuccess) return e;
    const int64_t tiles = (d.dim + kSegTile - 1) / kSegTile;
    const unsigned tile_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles + 3) / 4, 16384));
    hipLaunchKernelGGL(k_glm_seg_tiles, dim3(tile_grid), dim3(256), 0, st, d, win, batch, coef, g, head, items, units, item_cap,
                       unit_cap, count);
    if (item_cap > 0) {
        const unsigned wide_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((unit_cap + 3) / 4, 2048));
        hipLaunchKernelGGL(k_glm_seg_wide, dim3(wide_grid), dim3(256), 0, st, d, win, batch, coef, g, head, items, units, partial,
                           count);
        if (d.nnz >= kSegSplitAt) {
            const unsigned red_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((item_cap + 255) / 256, 1024));
            hipLaunchKernelGGL(k_glm_seg_reduce, dim3(red_grid), dim3(256), 0, st, g, head, items, partial, count);
        }
    }
    return hipGetLastError();
}

}  // namespace skml
