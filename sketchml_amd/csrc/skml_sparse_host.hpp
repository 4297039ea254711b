// skml_sparse_host.hpp -- what the sparse host files (skml_sparse_*.cpp) share: the library-owned
// payload and its owner while it is being built, the scratch slots, and the drivers that more than
// one file calls.  Never included by a .hip.
#pragma once
#include <atomic>
#include <vector>

#include "skml_host.hpp"
#include "skml_sparse_sum_plan.hpp"
#include "skml_sparse_wire.hpp"

// =============================================================================================
// library-owned sparse payload
// =============================================================================================
struct skml_sparse {
    int device = 0;
    int64_t nnz = 0;
    skml_params params{};
    void* qpayload = nullptr;  // dense payload of the values' quantizer (header, splits, codes)
    size_t qbytes = 0;
    skml_dense_header hdr{};
    std::vector<double> splits;
    std::vector<double> qvalues;  // SparseVectorCompressor.quantValues (getValues, timesBy'd)
    skml::SpGroups g{};         // host copy (complete after encode)
    void* block = nullptr;      // encode: one pooled device block holding everything below
    size_t block_cap = 0;
    skml::SpGroups* g_dev = nullptr;  // device copy
    int32_t* tables = nullptr;  // all groups' MinMaxSketch tables, rows x cols each
    int64_t ncells = 0;
    void* tnar = nullptr;       // their exact narrow image (tnar_width_for), or nullptr; in the block
    int tnar_width = 0;         // 8 or 16 bits a cell
    double* qv_dev = nullptr;   // quantValues on the device (in the block), valid while qv_dev_ok:
    bool qv_dev_ok = false;     // written by the encode / import, stale after timesBy until re-uploaded
    uint64_t* flag_words = nullptr;  // concatenated DeltaAdaptive flag streams
    uint64_t* delta_words = nullptr;
    int64_t flag_bits = 0, delta_bits = 0;
    int64_t n_flag_words = 0, n_delta_words = 0;
    // MinMaxSketch tables' HuffmanEncoder (built on the first serialisation)
    bool huff_done = false;
    std::vector<std::vector<skml::HuffItem>> huff_items;  // per group, ascending value
    std::vector<int64_t> huff_bit0, huff_bits;            // per group stream range
    uint64_t* huff_words = nullptr;
    int64_t n_huff_words = 0;
    void* wire_dev = nullptr;   // the serialised field stream on the device (built once; the
    size_t wire_bytes = 0;      // encoded state is immutable: timesBy scales quantValues only)
};

namespace skml {

// scratch slots (device)
enum {
    kSlotTiles = 0,
    kSlotGKeys,
    kSlotGBins,
    kSlotNeed,
    kSlotCells,
    kSlotSmall,  // hist + err + gpre + run offsets
    kSlotEndPos,
    kSlotDelta,
    kSlotK1,
    kSlotB1,
    kSlotStatus,
    kSlotCellIdx,
    kSlotTileOff,
    kSlotCKeys,     // toSparse output of skml_sparse_encode_f32
    kSlotCVals,
    kSlotDeltaEnc,  // standalone DeltaAdaptiveEncoder: group table + stream words
    kSlotWire,      // readObject: the device copy of the field stream
    kSlotWireMeta,  // the wire kernels' section tables and small results
    kSlotNarrowTab, // the MinMax query's narrow table image
    kSlotRsMerge,   // one-pass Sort.merge: RsInfo + the runs' key-range bounds
    kSlotLookback,  // the restore's look-back statuses (lengths + deltas in one pass)
    kSlotAggAcc,    // Gradient.sum returned as float / bf16 / fp16: the double sum between tile launches
    kSlotCount_,
};
static_assert(kSlotCount_ <= kScratchSlots, "scratch slots");

template <class T>
T* scratch(skml_ctx* c, int slot, size_t count) {
    return reinterpret_cast<T*>(ctx_scratch(c, slot, sizeof(T) * (count ? count : 1)));
}

// A failed check of skml_sparse_wire.hpp, reported: its text becomes skml_last_error.
inline int report(const WireStatus& st) { return st.code ? fail(st.code, "%s", st.msg) : SKML_OK; }

// The short form of HIP_TRY that the payload builders' error texts use.
#define SP_TRY(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return skml::fail(SKML_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ---- skml_sparse_payload.cpp ----
// Pooled device blocks of encoded payloads: the smallest pooled block of `dev` holding `bytes`
// (or a new one; nullptr when out of memory), and its return to the pool.
void* block_get(int dev, size_t bytes, size_t* cap);
void block_put(int dev, void* p, size_t cap);
// Frees the payload and what it owns (its block goes back to the pool).
void sparse_release(skml_sparse* s);
// The host table is edited between uploads, so each upload completes before returning.
int upload_groups(skml_ctx* c, skml_sparse* s);
int sync_to_host(skml_ctx* c, void* dst, const void* src, size_t bytes);
// Exclusive column scans of a [tiles][K] table; column totals copied to `totals` (host).
int scan_tiles(skml_ctx* c, uint64_t* sums, int64_t tiles, int K, uint64_t* totals);
extern thread_local int t_merge_path;        // skml_debug_sparse_merge_path
extern std::atomic<int> g_fail_cellbuf;      // skml_debug_sparse_scratch_fail
extern std::atomic<int64_t> g_sum_budget;    // skml_debug_sparse_sum_budget: 0 = kSumBudget
extern thread_local int32_t t_sum_batches, t_sum_launches;  // skml_debug_sparse_sum_path

// A payload under construction.  Until release() hands it to the caller, leaving the scope waits
// for the streams that may still use its memory (a pooled block must have no pending user) and
// frees it, so no return between the allocation and `*out = s` can skip the release.
struct PayloadOwner {
    skml_sparse* s;
    hipStream_t st, side = nullptr;  // side: a forked chain's stream, once it exists
    PayloadOwner(skml_sparse* payload, hipStream_t stream) : s(payload), st(stream) {}
    PayloadOwner(const PayloadOwner&) = delete;
    PayloadOwner& operator=(const PayloadOwner&) = delete;
    ~PayloadOwner() {
        if (!s) return;
        (void)hipStreamSynchronize(st);
        if (side) (void)hipStreamSynchronize(side);
        sparse_release(s);
    }
    void release(skml_sparse** out) {
        *out = s;
        s = nullptr;
    }
};

// A temporary device allocation: freed, after the stream that used it has drained, on every way
// out of the scope.
struct DevTemp {
    void* p = nullptr;
    hipStream_t st;
    explicit DevTemp(hipStream_t stream) : st(stream) {}
    DevTemp(const DevTemp&) = delete;
    DevTemp& operator=(const DevTemp&) = delete;
    ~DevTemp() {
        if (!p) return;
        (void)hipStreamSynchronize(st);
        (void)hipFree(p);
    }
    void* release() {
        void* q = p;
        p = nullptr;
        return q;
    }
};

// ---- skml_sparse_restore.cpp ----
// DecodeValues: Gradient.sum's restore writes narrow bins (bw bytes: 1 for bin_num <= 256, else 2)
// into gb for the tiled sum, which looks quantValues up itself; a bin outside the nq values sets *err.
// rb: the tiles' run bounds, written by the query too (rb.bounds nullptr: not).
struct DecodeValues {
    int nq;
    void* gb;
    int bw;
    unsigned* err;
    RunBoundsOut rb;
};
// DeltaAdaptive decode of all groups + MinMax query: grouped keys/bins into gk/gb.
int decode_groups(skml_ctx* c, const skml_sparse* s, int32_t* gk, int32_t* gb, bool query,
                  const DecodeValues* dv = nullptr, const RunBoundsOut* rbo = nullptr);
// Sort.merge (util/Sort.java:362-379) of the groups' (key, bin) runs: rounds of pairwise stable
// merges on the device; keys and bins land in keys_out / bins_out.
int merge_groups(skml_ctx* c, const skml_sparse* s, int32_t* gk, int32_t* gb, int32_t* keys_out, int32_t* bins_out);
// Sort.merge's one-pass form: its scratch (RsInfo + the runs' key-range bounds) taken and RsInfo
// zeroed up front, so the fill runs while the restore's first kernels are still being queued;
// m->info stays nullptr when the one-pass form will not run (one run, or the rounds forced through
// skml_debug_form).
struct RsMerge {
    RsInfo* info = nullptr;
    int32_t* bounds = nullptr;
    bool by_query = false;  // the key query writes the bounds (query_bounds); else k_rs_bounds
    RunBoundsOut query_bounds() {
        by_query = info && form(SKML_FORM_RUN_BOUNDS) != 1;
        return RunBoundsOut{by_query ? bounds : nullptr, 0, 0, kRsBits, info};
    }
};
int rs_merge_prepare(skml_ctx* c, const skml_sparse* s, RsMerge* m);
// The one-pass merge (launch_rs_merge) into keys_out and out (vkind: 0 int32 bins, 1 float / 2
// double quantValues[bin]).  *pending: a pinned word that is non-zero after the stream
// synchronises if the input was not regular (or held a bin outside quantValues) and merge_groups
// must run instead; nullptr when the one-pass form did not run.
int rs_merge_start(skml_ctx* c, const skml_sparse* s, const RsMerge& m, const int32_t* gk, const int32_t* gb,
                   int32_t* keys_out, void* out, int vkind, const double* qv, int nq, volatile unsigned** pending);

}  // namespace skml
