// skml_dense_ref.cpp -- a dense payload to and from the reference's Java serialisation layout
// (big-endian binNum, n, splits, zeroIdx, min, max and the bins).
#include <cstring>
#include <vector>

#include "skml_host.hpp"

using namespace skml;

extern "C" {

static void put_be(uint8_t* p, uint64_t v, int nb) {
    for (int i = nb - 1; i >= 0; i--) {
        p[i] = (uint8_t)(v & 0xFF);
        v >>= 8;
    }
}
static uint64_t get_be(const uint8_t* p, int nb) {
    uint64_t v = 0;
    for (int i = 0; i < nb; i++) v = (v << 8) | p[i];
    return v;
}
static uint64_t dbl_bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

int skml_dense_serialize_ref(skml_ctx* c, const void* payload, uint8_t* buf, size_t cap, size_t* written) {
    skml_dense_header h;
    std::vector<double> sp(SKML_MAX_BINS);
    int st = skml_dense_info(c, payload, &h, sp.data(), SKML_MAX_BINS);
    if (st) return st;
    const int B = h.bin_num, ns = B - 1;
    const int width = B <= 256 ? 1 : (B <= 65536 ? 2 : 4);
    const size_t head = 4 + 4 + 8 * (size_t)ns + 4 + 8 + 8 + 4;
    const size_t total = head + (size_t)width * (size_t)h.n;
    if (written) *written = total;
    if (!buf) return SKML_OK;
    if (cap < total) return fail(SKML_E_ARG, "buffer capacity %zu < %zu", cap, total);
    uint8_t* p = buf;
    put_be(p, (uint32_t)B, 4); p += 4;
    put_be(p, (uint32_t)h.n, 4); p += 4;
    for (int i = 0; i < ns; i++) { put_be(p, dbl_bits(sp[i]), 8); p += 8; }
    put_be(p, (uint32_t)h.zero_idx, 4); p += 4;
    put_be(p, dbl_bits(h.min), 8); p += 8;
    put_be(p, dbl_bits(h.max), 8); p += 8;
    put_be(p, (uint32_t)h.n, 4); p += 4;
    if (h.n > 0) {
        const size_t body = (size_t)width * (size_t)h.n;
        if ((st = reserve(c, c->stage, body, body, "stage buffer"))) return st;
        HIP_TRY(launch_ref_body(c->stream, payload, (uint8_t*)c->stage.p, h.n, width));
        HIP_TRY(hipMemcpyAsync(p, c->stage.p, body, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SKML_OK;
}

int skml_dense_deserialize_ref(skml_ctx* c, const uint8_t* buf, size_t len, void* payload, size_t cap) {
    if (!c || !buf || !valid_payload_ptr(payload)) return fail(SKML_E_ARG, "bad arguments");
    if (len < 8) return fail(SKML_E_ARG, "truncated stream");
    const uint8_t* p = buf;
    const int32_t B = (int32_t)get_be(p, 4);
    const int32_t n = (int32_t)get_be(p + 4, 4);
    if (B < 2 || B > SKML_MAX_BINS || n < 0) return fail(SKML_E_ARG, "bad binNum %d / n %d", B, n);
    const int ns = B - 1;
    const int width = B <= 256 ? 1 : (B <= 65536 ? 2 : 4);
    const size_t head = 4 + 4 + 8 * (size_t)ns + 4 + 8 + 8 + 4;
    if (len < head) return fail(SKML_E_ARG, "truncated stream");
    p += 8;
    std::vector<double> sp(ns);
    for (int i = 0; i < ns; i++) {
        uint64_t u = get_be(p, 8);
        std::memcpy(&sp[i], &u, 8);
        p += 8;
    }
    skml_dense_header h;
    std::memset(&h, 0, sizeof(h));
    h.magic = SKML_DENSE_MAGIC;
    h.status = SKML_OK;
    h.zero_idx = (int32_t)get_be(p, 4); p += 4;
    uint64_t u = get_be(p, 8); std::memcpy(&h.min, &u, 8); p += 8;
    u = get_be(p, 8); std::memcpy(&h.max, &u, 8); p += 8;
    const int32_t nb = (int32_t)get_be(p, 4); p += 4;
    if (nb != n || len < head + (size_t)width * (size_t)n) return fail(SKML_E_ARG, "truncated bins");
    if (cap < skml_dense_payload_bytes(n, B)) return fail(SKML_E_ARG, "payload too small");
    // Quantizer.findZeroIdx only yields indices of bins (Quantizer.java:74-85)
    if (h.zero_idx < 0 || h.zero_idx >= B) return fail(SKML_E_ARG, "zeroIdx %d outside [0, %d)", h.zero_idx, B);
    h.n = n;
    h.bin_num = B;
    h.code_bits = code_bits_for(B);
    h.req_bins = B;
    h.codes_offset = (int64_t)dense_codes_offset(B);
    HIP_TRY(hipSetDevice(c->device));
    const size_t body = align_up((size_t)width * (size_t)n, 16);
    int st = reserve(c, c->stage, body + 16, body + 16, "stage buffer");
    if (st) return st;
    int* bad = reinterpret_cast<int*>((char*)c->stage.p + body);
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), c->stream));
    HIP_TRY(hipMemcpyAsync(payload, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    if (ns) HIP_TRY(hipMemcpyAsync((char*)payload + kHeaderBytes, sp.data(), sizeof(double) * ns,
                                   hipMemcpyHostToDevice, c->stream));
    if (n) {
        HIP_TRY(hipMemcpyAsync(c->stage.p, p, (size_t)width * (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_pack_ref(c->stream, (const uint8_t*)c->stage.p, width, n, payload, bad));
    }
    int nbad = 0;
    HIP_TRY(hipMemcpyAsync(&nbad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nbad) {
        // leave no usable payload behind (on the context's stream, never the null stream)
        const uint32_t zero = 0;
        HIP_TRY(hipMemcpyAsync(payload, &zero, sizeof(zero), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fail(SKML_E_ARG, "bin outside [0, %d) in the stream", B);
    }
    return SKML_OK;
}

}  // extern "C"
