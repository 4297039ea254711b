// skml_zip_api.cpp -- host side of ZipGradient's ZipMLQuantizer of the C ABI (include/skml.h;
// ml/gradient/ZipGradient.scala:61-139): sort, prefix sums, the split search's rounds.
#include <cstring>

#include "skml_host.hpp"

using namespace skml;

namespace {
// The scratch of a call: the context's ZipML workspace, grow-only like its other workspaces (a
// fresh 9.7 GB allocation for 2^28 values costs the driver about half a second, so it is kept; it
// goes with the context) and sized exactly.  Growing waits for the stream, then frees and allocates.
int zip_alloc(skml_ctx* c, int64_t n, int wide, int own_prefix, ZipScratch* s) {
    const size_t bytes = zip_scratch_layout(n, wide, own_prefix, nullptr, nullptr);
    if (int st = reserve(c, c->zip_ws, bytes, bytes, "ZipML scratch")) return st;
    zip_scratch_layout(n, wide, own_prefix, s, (char*)c->zip_ws.p);
    return SKML_OK;
}

int zip_read_state(skml_ctx* c, const ZipScratch& s, ZipState* out) {
    void* pin = skml::ctx_pinned(c, sizeof(ZipState));
    if (!pin) return fail(SKML_E_OOM, "pinned staging of the ZipML state");
    HIP_TRY(hipMemcpyAsync(pin, s.state, sizeof(ZipState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(out, pin, sizeof(ZipState));
    return SKML_OK;
}

// The sorted copy (as doubles) and, when r is not null, the two prefix sums: the encode's first
// stage and the debug hooks' whole work.  Synchronises (the NaN / infinity flag).
int zip_prefix(skml_ctx* c, const void* x, int wide, int64_t n, const ZipScratch& s, double* sorted, double* r,
               double* t) {
    HIP_TRY(hipMemsetAsync(s.state, 0, sizeof(ZipState), c->stream));
    HIP_TRY(launch_zip_sort(c->stream, x, wide, n, s, sorted));
    if (r) HIP_TRY(launch_zip_scan(c->stream, sorted, n, r, t, s));
    ZipState hs;
    if (int st = zip_read_state(c, s, &hs)) return st;
    if (hs.bad) return fail(SKML_E_NAN, "Encounter NaN or infinite value");
    return SKML_OK;
}

int zip_check_n(skml_ctx* c, const void* x, int64_t n) {
    if (n < 2 || n > 0x7FFFFFFFLL) return fail(SKML_E_ARG, "n=%lld outside [2, 2^31 - 1]", (long long)n);
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!x || ((uintptr_t)x) % 16 != 0) return fail(SKML_E_ARG, "input must be a 16-byte aligned device pointer");
    return SKML_OK;
}

const char* const kZipNoProgressMsg =
    "ZipML split search makes no progress (%lld splits stay %lld): the reference's loop does not terminate on this input";

int zip_encode_x(skml_ctx* c, const void* x, int wide, int64_t n, int32_t bins, void* payload, size_t cap) {
    // the argument checks come first and need no device
    if (bins < kZipMinBins || bins > SKML_MAX_BINS)
        return fail(SKML_E_ARG, "ZipML bin number %d outside [%d, %d] (2 and 3 select the 0-th largest error)", bins,
                    kZipMinBins, SKML_MAX_BINS);
    if (int st = zip_check_n(c, x, n)) return st;
    if (!valid_payload_ptr(payload)) return fail(SKML_E_ARG, "payload must be 256-byte aligned");
    if (cap < skml_dense_payload_bytes(n, bins))
        return fail(SKML_E_ARG, "payload capacity %zu < %zu", cap, skml_dense_payload_bytes(n, bins));
    HIP_TRY(hipSetDevice(c->device));
    Workspace w;  // the quantize LUT
    int st;
    if ((st = ensure_ws(c, 0, &w))) return st;
    ZipScratch s;
    if ((st = zip_alloc(c, n, wide, 1, &s))) return st;
    ZipState hs;
    {
        KernelTimer kt(c, SKML_K_SUMMARY);
        if ((st = zip_prefix(c, x, wide, n, s, s.sorted, s.r, s.t))) return st;
        int64_t sn = n;
        const int32_t* idx = nullptr;
        int32_t* bufs[2] = {s.idx_a, s.idx_b};
        int cur = 0, rounds = 0;
        while (sn > bins && sn > kZipTail) {
            HIP_TRY(launch_zip_round(c->stream, idx, bufs[cur], sn, n, bins, s.r, s.t, s));
            if ((st = zip_read_state(c, s, &hs))) return st;
            const int64_t next = sn / 2 + hs.kept;  // an odd splitNum's last singleton is dropped
            if (hs.kept < 0 || next >= sn) return fail(SKML_E_ARG, kZipNoProgressMsg, (long long)sn, (long long)next);
            idx = bufs[cur];
            cur ^= 1;
            sn = next;
            rounds++;
        }
        HIP_TRY(launch_zip_finish(c->stream, idx, sn, n, bins, s.r, s.t, s.sorted, s));
        if ((st = zip_read_state(c, s, &hs))) return st;
        if (hs.status == kZipThrZero) return fail(SKML_E_ARG, "ZipML round with thrNum 0");
        if (hs.status == kZipNoProgress)
            return fail(SKML_E_ARG, kZipNoProgressMsg, (long long)hs.bin_num, (long long)hs.bin_num);
        if (hs.bin_num < 2 || hs.bin_num > bins) return fail(SKML_E_STATE, "ZipML split search ended with %d bins", hs.bin_num);
        c->zip_rounds = rounds + hs.rounds;
        HIP_TRY(launch_set_splits(c->stream, payload, n, s.splits, hs.bin_num - 1, hs.mn, hs.mx, bins, w.lut));
    }
    {
        KernelTimer kt(c, SKML_K_QUANTIZE);
        if (wide) HIP_TRY(launch_quantize64(c->stream, static_cast<const double*>(x), n, payload, w.lut, nullptr, bins));
        else HIP_TRY(launch_quantize(c->stream, &c->qres, x, n, payload, w.lut, bins));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SKML_OK;
}

int zip_debug_prefix_x(skml_ctx* c, const void* x, int wide, int64_t n, double* sorted, double* r, double* t) {
    if (int st = zip_check_n(c, x, n)) return st;
    if (!sorted || (r == nullptr) != (t == nullptr)) return fail(SKML_E_ARG, "sorted_dev is NULL, or one of r_dev / t_dev");
    HIP_TRY(hipSetDevice(c->device));
    ZipScratch s;
    if (int st = zip_alloc(c, n, wide, 0, &s)) return st;
    KernelTimer kt(c, SKML_K_SUMMARY);
    return zip_prefix(c, x, wide, n, s, sorted, r, t);
}
}  // namespace

extern "C" {

size_t skml_zip_workspace_bytes(int64_t n, int32_t fp64) {
    if (n < 2 || n > 0x7FFFFFFFLL) return 0;
    return zip_scratch_layout(n, fp64 ? 1 : 0, 1, nullptr, nullptr);
}

int skml_debug_zip_rounds(skml_ctx* c) { return c ? c->zip_rounds : -1; }

int skml_zip_release_workspace(skml_ctx* c) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!c->zip_ws.p) return SKML_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    release(c->zip_ws);
    return SKML_OK;
}

int skml_zip_encode_f32(skml_ctx* c, const float* x, int64_t n, int32_t bin_num, void* payload, size_t cap) {
    return zip_encode_x(c, x, 0, n, bin_num, payload, cap);
}

int skml_zip_encode_f64(skml_ctx* c, const double* x, int64_t n, int32_t bin_num, void* payload, size_t cap) {
    return zip_encode_x(c, x, 1, n, bin_num, payload, cap);
}

int skml_debug_zip_prefix_f32(skml_ctx* c, const float* x, int64_t n, double* sorted, double* r, double* t) {
    return zip_debug_prefix_x(c, x, 0, n, sorted, r, t);
}

int skml_debug_zip_prefix_f64(skml_ctx* c, const double* x, int64_t n, double* sorted, double* r, double* t) {
    return zip_debug_prefix_x(c, x, 1, n, sorted, r, t);
}

}  // extern "C"
