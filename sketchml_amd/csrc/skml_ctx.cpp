// skml_ctx.cpp -- the context behind the C ABI (include/skml.h): creation and teardown, the
// thread's error message, the kernel-form selections, per-kernel timing, the grow-only buffers
// and the side context.  No codec lives here.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "skml_host.hpp"

using namespace skml;

static thread_local std::string g_err;

namespace skml {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int reserve(skml_ctx* c, DevBuf& b, size_t bytes, size_t cap_for_bytes, const char* what, bool* grew, bool pinned) {
    if (grew) *grew = false;
    if (bytes <= b.cap) return SKML_OK;
    if (b.p) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        void* old = b.p;
        b = DevBuf{};  // empty before anything below can fail: p == nullptr implies cap == 0
        HIP_TRY(pinned ? hipHostFree(old) : hipFree(old));
    }
    void* p = nullptr;
    if ((pinned ? hipHostMalloc(&p, cap_for_bytes, hipHostMallocDefault) : hipMalloc(&p, cap_for_bytes)) != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable
        return fail(SKML_E_OOM, "%s of %zu B", what, cap_for_bytes);
    }
    b.p = p;
    b.cap = cap_for_bytes;
    if (grew) *grew = true;
    return SKML_OK;
}

void release(DevBuf& b, bool pinned) {
    if (b.p) (void)(pinned ? hipHostFree(b.p) : hipFree(b.p));
    b = DevBuf{};
}

// skml_debug_form's process-wide selections (read once per launch decision, no environment)
static std::atomic<int> g_form[SKML_FORM_COUNT];
int form(int id) { return id >= 0 && id < SKML_FORM_COUNT ? g_form[id].load(std::memory_order_relaxed) : 0; }
}  // namespace skml

// The forms whose kernels only the A/B build (-DSKML_AB, sketchml_amd/lib_ab) carries: measured
// slower than the default, kept for the A/B tools and the tests that load that build.
static bool ab_only_form(int id, int v) {
    switch (id) {
        case SKML_FORM_LEAF_SPLIT: return v == 1 || v >= 3;
        case SKML_FORM_DECODE_SUM: return v == 2;
        case SKML_FORM_RS_ROUNDS: return v == 2;
        case SKML_FORM_DEC_ROWS_SERIAL: return v == 2;
        case SKML_FORM_AGG_TILES: return v >= 2;
        case SKML_FORM_RUN_BOUNDS: return v != 0;
        case SKML_FORM_DEC_LOOKBACK: return v != 0;
        default: return false;
    }
}

extern "C" int skml_debug_form(int id, int value) {
    if (id < 0 || id >= SKML_FORM_COUNT) return -1;
#ifndef SKML_AB
    if (ab_only_form(id, value)) return -2;
#else
    (void)ab_only_form;
#endif
    return g_form[id].exchange(value);
}

extern "C" int skml_build_flags(void) {
#ifdef SKML_AB
    return SKML_BUILD_AB;
#else
    return 0;
#endif
}

static void build_jump_table(std::vector<uint64_t>& tab) {
    tab.assign(4 * 256 * 2, 0);
    uint64_t base_a = kLcgMult, base_c = kLcgAdd;  // J_1
    for (int lvl = 0; lvl < 4; lvl++) {
        uint64_t a = 1, c = 0;  // J_0
        for (int b = 0; b < 256; b++) {
            tab[(lvl * 256 + b) * 2] = a;
            tab[(lvl * 256 + b) * 2 + 1] = c;
            // J_{(b+1) * 256^lvl} = J_base o J_{b * 256^lvl}
            c = (base_a * c + base_c) & kLcgMask;
            a = (base_a * a) & kLcgMask;
        }
        // next base = J_base^256
        uint64_t na = 1, nc = 0;
        for (int i = 0; i < 256; i++) {
            nc = (base_a * nc + base_c) & kLcgMask;
            na = (base_a * na) & kLcgMask;
        }
        base_a = na;
        base_c = nc;
    }
}

extern "C" {

void skml_params_default(skml_params* p) {
    p->bin_num = 256;
    p->group_num = 8;
    p->row_num = 2;
    p->dedup = 1;
    p->col_ratio = 0.3;
    p->seed = 0;
    p->hash_seed = 0;
    p->quant_type = SKML_QUANTILE;
    p->parallelism = 1;
}

const char* skml_last_error(void) { return g_err.c_str(); }
const char* skml_version(void) { return "skml-mi355x 0.1 (gfx950)"; }

int skml_ctx_create(int device, void* hip_stream, skml_ctx** out) {
    if (!out) return fail(SKML_E_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(SKML_E_ARG, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));
    skml_ctx* c = new skml_ctx();
    c->device = device;
    if (hip_stream != SKML_STREAM_OWN) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return fail(SKML_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        c->own_stream = true;
    }
    std::vector<uint64_t> tab;
    build_jump_table(tab);
    // Uploaded on the context's own stream from its pinned staging buffer, complete before the
    // context exists.  A hipMemcpy goes through the null stream, and an async copy out of pageable
    // memory waits for it too while the runtime registers the host pages: either way the creation
    // (and the first batched encode, which creates the side context) stalled behind whatever the
    // null stream was running.
    const size_t tab_bytes = tab.size() * sizeof(uint64_t);
    hipError_t e = hipMalloc(&c->jump_tab, tab_bytes);
    void* pin = e == hipSuccess ? skml::ctx_pinned(c, tab_bytes) : nullptr;
    if (e == hipSuccess && !pin) e = hipErrorOutOfMemory;
    if (e == hipSuccess) {
        std::memcpy(pin, tab.data(), tab_bytes);
        e = hipMemcpyAsync(c->jump_tab, pin, tab_bytes, hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        skml_ctx_destroy(c);
        return fail(SKML_E_HIP, "jump table: %s", hipGetErrorString(e));
    }
    *out = c;
    return SKML_OK;
}

int skml_ctx_destroy(skml_ctx* c) {
    if (!c) return SKML_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->jump_tab) (void)hipFree(c->jump_tab);
    for (DevBuf* b : {&c->ws, &c->ws64, &c->ranks, &c->stage, &c->sk, &c->zip_ws, &c->opt_ws, &c->glm_ws}) release(*b);
    for (DevBuf& b : c->scratch) release(b);
    release(c->pinned, true);
    if (c->side) skml_ctx_destroy(c->side);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_leaf) (void)hipEventDestroy(c->ev_leaf);
    if (c->ev_fork2) (void)hipEventDestroy(c->ev_fork2);
    if (c->ev_join2) (void)hipEventDestroy(c->ev_join2);
    if (c->ev_switch) (void)hipEventDestroy(c->ev_switch);
    if (c->fx_part) (void)hipFree(c->fx_part);
    for (int k = 0; k < SKML_K_COUNT; k++)
        for (hipEvent_t e : c->ev[k]) (void)hipEventDestroy(e);
    if (c->hword) (void)hipHostFree(c->hword);
    destroy_host_path(c);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return SKML_OK;
}

int skml_ctx_sync(skml_ctx* c) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SKML_OK;
}

int skml_ctx_set_timing(skml_ctx* c, int mask) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    c->timing = mask;
    return SKML_OK;
}

int skml_ctx_reset_stats(skml_ctx* c) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < SKML_K_COUNT; k++) c->ev_used[k] = 0;
    return SKML_OK;
}

int skml_ctx_kernel_stats(skml_ctx* c, int kid, int64_t* launches, double* total_ms) {
    if (!c || kid < 0 || kid >= SKML_K_COUNT) return fail(SKML_E_ARG, "bad kernel id");
    HIP_TRY(hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (size_t i = 0; i + 1 < c->ev_used[kid]; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[kid][i], c->ev[kid][i + 1]));
        tot += ms;
    }
    if (launches) *launches = (int64_t)(c->ev_used[kid] / 2);
    if (total_ms) *total_ms = tot;
    return SKML_OK;
}

int skml_ctx_set_stream(skml_ctx* c, void* hip_stream) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (hip_stream == SKML_STREAM_OWN) return fail(SKML_E_ARG, "SKML_STREAM_OWN is only valid at creation");
    hipStream_t next = (hipStream_t)hip_stream;
    if (next == c->stream) return SKML_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (c->own_stream) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipStreamDestroy(c->stream));
        c->own_stream = false;
    } else {
        // the context's workspace (merge arrival counter, LUT, stage, scratch) is reused by the next
        // call: order the new stream after everything still queued on the old one
        if (!c->ev_switch) HIP_TRY(hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->ev_switch, c->stream));
        HIP_TRY(hipStreamWaitEvent(next, c->ev_switch, 0));
    }
    c->stream = next;
    return SKML_OK;
}

}  // extern "C"

namespace skml {

// The side context: a child context on its own stream, created at high priority (HIP keeps
// hardware queues per priority, so the two never share a queue; with GPU_MAX_HW_QUEUES = 4, a
// normal-priority stream created after the framework's own streams was measured to share one and
// serialise the lanes).  Used by the batched encode and the sparse encode's DeltaAdaptive chain.
int ensure_side(skml_ctx* c) {
    if (c->side) return SKML_OK;
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi));
    int st = skml_ctx_create(c->device, s, &c->side);
    if (st) {
        (void)hipStreamDestroy(s);
        return st;
    }
    c->side->own_stream = true;
    HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    return SKML_OK;
}

int ctx_side_fork(skml_ctx* c, hipStream_t* side, hipEvent_t* fork, hipEvent_t* join) {
    // SKML_SERIAL=1 (profiling): no fork, every kernel runs alone on the caller's stream
    static const bool serial = [] {
        const char* e = std::getenv("SKML_SERIAL");
        return e && e[0] == '1';
    }();
    if (serial) return SKML_E_STATE;
    if (int st = ensure_side(c)) return st;
    if (!c->ev_fork2) HIP_TRY(hipEventCreateWithFlags(&c->ev_fork2, hipEventDisableTiming));
    if (!c->ev_join2) HIP_TRY(hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming));
    *side = c->side->stream;
    *fork = c->ev_fork2;
    *join = c->ev_join2;
    return SKML_OK;
}

void* ctx_scratch(skml_ctx* c, int slot, size_t bytes) {
    if (slot < 0 || slot >= kScratchSlots) return nullptr;
    if (bytes == 0) bytes = 256;
    if (reserve(c, c->scratch[slot], bytes, align_up(bytes + bytes / 8, 256), "scratch slot")) return nullptr;
    return c->scratch[slot].p;
}

int64_t* ctx_host_word(skml_ctx* c) {
    if (!c->hword) {
        void* p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        c->hword = static_cast<int64_t*>(p);
    }
    return c->hword;
}

void* ctx_pinned(skml_ctx* c, size_t bytes) {
    if (reserve(c, c->pinned, bytes, align_up(bytes + bytes / 8 + 4096, 4096), "pinned staging", nullptr, true))
        return nullptr;
    return c->pinned.p;
}

}  // namespace skml
