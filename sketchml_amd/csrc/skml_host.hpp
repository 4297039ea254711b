// skml_host.hpp -- what the host translation units (*.cpp) share: the context, its grow-only
// buffers, the error state and the per-kernel timer.  Never included by a .hip.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "skml_internal.h"
#include "skml_sparse.h"

namespace skml {

// Sets the calling thread's skml_last_error message and returns `code` (skml_ctx.cpp).
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return skml::fail(SKML_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                              __FILE__, __LINE__);                                                \
    } while (0)

// A grow-only block of device (or pinned host) memory owned by a context.  p == nullptr implies
// cap == 0: reserve is the only place that sets either.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};
constexpr int kScratchSlots = 24;

}  // namespace skml

struct skml_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint64_t* jump_tab = nullptr;  // device, 4 x 256 x (A^m, C_m)
    skml::DevBuf ws;    // dense workspace
    skml::DevBuf ws64;  // fp64 sketch workspace
    // rank table cache for (n, bin_num): HeapQuantileSketch.getQuantiles' curFrac ranks
    skml::DevBuf ranks;
    int64_t ranks_n = -1;
    int ranks_bins = -1;
    // batched encode: a child context (own high-priority stream and workspace) and its events
    skml_ctx* side = nullptr;
    hipEvent_t ev_join = nullptr, ev_leaf = nullptr;
    hipEvent_t ev_fork2 = nullptr, ev_join2 = nullptr;  // sparse encode: its side-stream chain
    hipEvent_t after_leaf = nullptr;  // when set, recorded right after the next leaf launch
    hipEvent_t ev_switch = nullptr;   // skml_ctx_set_stream: orders the new stream after the old one
    skml::QuantResidency qres;  // quantize pass: resident workgroups per CU, per kernel form
    skml::DevBuf sk;  // parallelQuantize: slice records + the merged sketch's export
    // FixedPointGradient: the workgroup partials of the sum of squares (kFxMaxParts, allocated once)
    skml::FxPartial* fx_part = nullptr;
    skml::DevBuf zip_ws;  // ZipMLQuantizer: keys, sorted copy, prefix sums, errors, splitIndex
    int zip_rounds = 0;   // halving rounds of the last successful ZipML encode (skml_debug_zip_rounds)
    skml::DevBuf opt_ws;  // optimiser step: the live counter of SKML_OPT_AUTO
    skml::DevBuf glm_ws;  // mini-batch gradient: live counter, objLoss, and coef / loss_j when the caller keeps none
    skml::DevBuf stage;   // staging
    // sparse path: device scratch slots and pinned host staging
    skml::DevBuf scratch[skml::kScratchSlots];
    skml::DevBuf pinned;
    // one coherent, device-mapped host word: a kernel publishes a count there (the compaction's
    // nnz) and the host polls it instead of a copy + stream synchronisation
    int64_t* hword = nullptr;
    // host-memory entry points (skml_dense_encode_host_f32 / _decode_host_f32): device copies of
    // the input / payload, two pinned staging buffers and a pool of host copy threads
    skml::DevBuf hx, hp, hk;
    void* hpin[2] = {nullptr, nullptr};
    hipEvent_t hev[2] = {nullptr, nullptr};
    struct CopyPool* pool = nullptr;
    // per-kernel event timing (skml_ctx_set_timing)
    int timing = 0;  // bit k: time kernel id k
    std::vector<hipEvent_t> ev[SKML_K_COUNT];  // start/stop pairs
    size_t ev_used[SKML_K_COUNT] = {};
};

namespace skml {

// Records a start event on construction and a stop event on destruction when timing is on.
struct KernelTimer {
    skml_ctx* c;
    int kid;
    bool on;
    KernelTimer(skml_ctx* ctx, int k) : c(ctx), kid(k), on((ctx->timing >> k) & 1) {
        if (!on) return;
        auto& v = c->ev[kid];
        if (c->ev_used[kid] + 2 > v.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
                on = false;
                return;
            }
            v.push_back(a);
            v.push_back(b);
        }
        (void)hipEventRecord(v[c->ev_used[kid]], c->stream);
    }
    ~KernelTimer() {
        if (!on) return;
        (void)hipEventRecord(c->ev[kid][c->ev_used[kid] + 1], c->stream);
        c->ev_used[kid] += 2;
    }
};

// ---- context services (skml_ctx.cpp) ----
// Makes b hold at least `bytes`.  When it is too small: waits for the context's stream if a block
// exists, frees it, clears p and cap, and allocates cap_for_bytes (the caller's slack policy for
// this need).  A failed allocation clears HIP's sticky error, leaves b empty and returns
// fail(SKML_E_OOM).  *grew tells the caller that the block is new (its contents undefined).
// pinned: page-locked host memory instead of device memory.
int reserve(skml_ctx* c, DevBuf& b, size_t bytes, size_t cap_for_bytes, const char* what, bool* grew = nullptr,
            bool pinned = false);
// Frees b's block (the caller has drained its users) and leaves b empty.
void release(DevBuf& b, bool pinned = false);
// the context's side stream (a high-priority child context) and two events for a fork / join;
// c->side is nullptr before the first fork
int ctx_side_fork(skml_ctx* c, hipStream_t* side, hipEvent_t* fork, hipEvent_t* join);
int ensure_side(skml_ctx* c);
// grow-only device scratch buffer `slot` (< kScratchSlots) of at least `bytes`; null on failure
void* ctx_scratch(skml_ctx* c, int slot, size_t bytes);
// pinned host staging of at least `bytes`; null on failure
void* ctx_pinned(skml_ctx* c, size_t bytes);
// the context's coherent, device-mapped host word (nullptr if it cannot be allocated)
int64_t* ctx_host_word(skml_ctx* c);
// frees the host-memory entry points' buffers, events and copy threads (skml_host_mem.cpp)
void destroy_host_path(skml_ctx* c);

// The caller's parameters, or the defaults in *def when it passed none.  clear_dedup: the defaults
// of parallelQuantize (the parallel and sharded entries), which does not deduplicate splits.
inline const skml_params* params_or_default(const skml_params* p, skml_params* def, bool clear_dedup) {
    if (p) return p;
    skml_params_default(def);
    if (clear_dedup) def->dedup = 0;
    return def;
}

// What the argument checks of the entries share: a named byte range of a caller's array (a NULL or empty
// range overlaps nothing), 8-byte alignment, and the largest length a Java int holds.
struct Range {
    const void* p;
    size_t bytes;
    const char* name;
};
inline bool overlap(const Range& a, const Range& b) {
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
inline bool aligned8(const void* p) { return ((uintptr_t)p) % 8 == 0; }
constexpr int64_t kJavaIntMax = 0x7FFFFFFFLL;

inline bool valid_payload_ptr(const void* p) { return p && (((uintptr_t)p) % 256 == 0); }

// ---- the dense workspace (skml_dense_api.cpp), also the home of the quantize LUT that the
// uniform, ZipML and fp64 encodes share ----
struct Workspace {
    unsigned* done;  // arrival counter of the fused summary (always at offset 0, self-resetting)
    LeafPartial* part;
    float* nodes6;
    float* roots;
    float* upA;
    float* upB;
    double* raw;
    QuantLut* lut;  // quantize bucket LUT, written by the summary / set-splits kernel
    UniPartial* uni;  // uniform quantizer partials
    int* qflags;      // fp64 quantize flags (bit 0: literal Quantizer.indexOf)
    uint8_t* ubits;   // compaction bits of the upper merge tree, drawn by the leaf
    LeafPartial* part_red;  // leaf partials reduced per first-pass merge workgroup
};
int ensure_ws(skml_ctx* ctx, int64_t chunks, Workspace* w);

// What every consumer of P gathered dense payloads checks first (skml_dense_decode_sum_*, the fused
// optimiser step): the context and the payload arguments, then the P headers read back through the
// pinned staging (synchronises): magic, status (SKML_E_NAN), n, code width, stride.
// *common_bits: the payloads' code width, 0 when they differ; *max_bins: the largest table.
int dense_sum_headers(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, int* common_bits,
                      int* max_bins);

// The same for P gathered fixed-point payloads (skml_fixed_decode_sum_f32, the fused fixed-point
// optimiser step; skml_fixed_api.cpp): magic, status (SKML_E_NAN), n, one num_bits, stride.
// *bits: the payloads' width.
int fixed_sum_headers(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, int* bits);

}  // namespace skml
