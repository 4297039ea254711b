// skml_fixed_api.cpp -- host side of the FixedPointGradient codec of the C ABI (include/skml.h;
// ml/gradient/FixedPointGradient.scala): encode, decode and the fused sum.
#include <cstring>

#include "skml_host.hpp"

using namespace skml;

extern "C" {

size_t skml_fixed_payload_bytes(int64_t n, int32_t num_bits) {
    if (n < 1 || n > 0x7FFFFFFFLL || num_bits < kFxMinBits || num_bits > kFxMaxBits) return 0;
    return kFxHeaderBytes + align_up((size_t)fixed_words(n, num_bits) * 8, 256);
}

static int fixed_encode_x(skml_ctx* c, const void* x, int wide, int64_t n, int32_t bits, int64_t seed, void* payload,
                          size_t cap) {
    // the argument checks come first and need no device
    if (bits >= 30) return fail(SKML_E_ARG, "Bit num out of range: %d", bits);  // FixedPointGradient.scala:16
    if (bits < kFxMinBits) return fail(SKML_E_ARG, "Bit num out of range: %d (one bit leaves max = 0 to divide by)", bits);
    if (n < 1 || n > 0x7FFFFFFFLL) return fail(SKML_E_ARG, "n=%lld outside [1, 2^31 - 1]", (long long)n);
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!x || ((uintptr_t)x) % 16 != 0) return fail(SKML_E_ARG, "input must be a 16-byte aligned device pointer");
    if (!valid_payload_ptr(payload)) return fail(SKML_E_ARG, "payload must be 256-byte aligned");
    if (cap < skml_fixed_payload_bytes(n, bits))
        return fail(SKML_E_ARG, "payload capacity %zu < %zu", cap, skml_fixed_payload_bytes(n, bits));
    HIP_TRY(hipSetDevice(c->device));
    if (!c->fx_part) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->fx_part), sizeof(FxPartial) * kFxMaxParts));
    {
        KernelTimer kt(c, SKML_K_SUMMARY);  // the reduction that makes the header, as the dense summary does
        HIP_TRY(launch_fixed_norm(c->stream, x, wide, n, bits, seed, c->fx_part, payload));
    }
    {
        KernelTimer kt(c, SKML_K_QUANTIZE);
        HIP_TRY(launch_fixed_quantize(c->stream, x, wide, n, payload, c->jump_tab));
    }
    return SKML_OK;
}

int skml_fixed_encode_f32(skml_ctx* c, const float* x, int64_t n, int32_t bits, int64_t seed, void* payload,
                          size_t cap) {
    return fixed_encode_x(c, x, 0, n, bits, seed, payload, cap);
}

int skml_fixed_encode_f64(skml_ctx* c, const double* x, int64_t n, int32_t bits, int64_t seed, void* payload,
                          size_t cap) {
    return fixed_encode_x(c, x, 1, n, bits, seed, payload, cap);
}

static int fixed_decode_x(skml_ctx* c, const void* payload, void* out, int wide, int64_t n) {
    if (!c || !valid_payload_ptr(payload) || n < 0 || (n > 0 && (!out || ((uintptr_t)out) % 16)))
        return fail(SKML_E_ARG, "bad decode arguments");
    HIP_TRY(hipSetDevice(c->device));
    KernelTimer kt(c, SKML_K_DECODE);
    HIP_TRY(launch_fixed_decode(c->stream, payload, out, wide, n));
    return SKML_OK;
}

int skml_fixed_decode_f32(skml_ctx* c, const void* payload, float* out, int64_t n) {
    return fixed_decode_x(c, payload, out, 0, n);
}

int skml_fixed_decode_f64(skml_ctx* c, const void* payload, double* out, int64_t n) {
    return fixed_decode_x(c, payload, out, 1, n);
}

int skml_fixed_decode_sum_f32(skml_ctx* c, const void* payloads, int32_t P, size_t stride, float* out, int64_t n,
                              double scale) {
    if (c && (!out || ((uintptr_t)out) % 16))
        return fail(SKML_E_ARG, "bad decode_sum arguments (P in [1,16], 256-B aligned payloads)");
    int bits = 0;
    if (const int st = fixed_sum_headers(c, payloads, P, stride, n, &bits)) return st;
    KernelTimer kt(c, SKML_K_DECODE_SUM);
    HIP_TRY(launch_fixed_decode_sum(c->stream, payloads, P, stride, out, n, scale, bits));
    return SKML_OK;
}

int skml_fixed_codes_i32(skml_ctx* c, const void* payload, int32_t* codes, int64_t n) {
    if (!c || !valid_payload_ptr(payload) || n < 0 || (n > 0 && !codes)) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_fixed_codes(c->stream, payload, codes, n));
    return SKML_OK;
}

int skml_fixed_times_by(skml_ctx* c, void* payload, double x) {
    if (!c || !valid_payload_ptr(payload)) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_fixed_times_by(c->stream, payload, x));
    return SKML_OK;
}

int skml_fixed_info(skml_ctx* c, const void* payload, skml_fixed_header* hdr) {
    if (!c || !valid_payload_ptr(payload) || !hdr) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    void* pin = skml::ctx_pinned(c, sizeof(*hdr));
    if (!pin) return fail(SKML_E_OOM, "pinned staging of the payload header");
    HIP_TRY(hipMemcpyAsync(pin, payload, sizeof(*hdr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(hdr, pin, sizeof(*hdr));
    if (hdr->magic != SKML_FIXED_MAGIC) return fail(SKML_E_STATE, "not a fixed-point payload");
    if (hdr->status == SKML_E_NAN) return fail(SKML_E_NAN, "NaN or infinite value, or a norm that is not finite or underflowed to 0");
    return hdr->status;
}

}  // extern "C"

int skml::fixed_sum_headers(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, int* bits) {
    if (!c || !valid_payload_ptr(payloads) || stride % 256 || P < 1 || P > 16 || n < 1)
        return fail(SKML_E_ARG, "bad decode_sum arguments (P in [1,16], 256-B aligned payloads)");
    HIP_TRY(hipSetDevice(c->device));
    // the headers come back through the context's pinned staging, as in dense_sum_headers
    skml_fixed_header* h = static_cast<skml_fixed_header*>(skml::ctx_pinned(c, sizeof(skml_fixed_header) * 16));
    if (!h) return fail(SKML_E_OOM, "pinned staging of the payload headers");
    for (int p = 0; p < P; p++)
        HIP_TRY(hipMemcpyAsync(h + p, static_cast<const char*>(payloads) + (size_t)p * stride, sizeof(skml_fixed_header),
                               hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int p = 0; p < P; p++) {
        if (h[p].magic != SKML_FIXED_MAGIC) return fail(SKML_E_STATE, "payload %d is not a fixed-point payload", p);
        if (h[p].status == SKML_E_NAN) return fail(SKML_E_NAN, "payload %d: NaN, infinite or underflowed input", p);
        if (h[p].status != SKML_OK) return fail(SKML_E_STATE, "payload %d has status %d", p, h[p].status);
        if (h[p].n != n)
            return fail(SKML_E_ARG, "payload %d holds %lld values, the sum %lld", p, (long long)h[p].n, (long long)n);
        if (h[p].num_bits != h[0].num_bits)
            return fail(SKML_E_ARG, "payload %d has %d bits, payload 0 %d", p, h[p].num_bits, h[0].num_bits);
        if (h[p].num_bits < kFxMinBits || h[p].num_bits > kFxMaxBits || h[p].words_offset != kFxHeaderBytes ||
            skml_fixed_payload_bytes(n, h[p].num_bits) > stride)
            return fail(SKML_E_ARG, "payload %d: inconsistent header or larger than the stride %zu", p, stride);
    }
    *bits = h[0].num_bits;
    return SKML_OK;
}
