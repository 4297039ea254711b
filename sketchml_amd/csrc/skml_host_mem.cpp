// skml_host_mem.cpp -- the host-memory entry points of the C ABI (include/skml.h): the path starts
// and ends in a JVM float[] / byte[] (north star).
// Pageable host memory is staged through two library-owned pinned buffers: host threads copy
// piece i+1 into one while the DMA engine moves piece i out of the other, so the pageable copy
// runs beside the PCIe transfer instead of before it.  Pinned caller memory (skml_host_alloc,
// e.g. behind a Java direct ByteBuffer) is transferred directly.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "skml_host.hpp"

using namespace skml;

struct CopyPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv, done_cv;
    std::function<void(int)> job;
    int parts = 0, next = 0, done = 0;
    uint64_t gen = 0;
    bool stop = false;
    explicit CopyPool(int n) {
        for (int i = 0; i < n; i++) th.emplace_back([this] { run(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
    void run() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(m);
        while (true) {
            cv.wait(lk, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            while (next < parts) {
                const int k = next++;
                lk.unlock();
                job(k);
                lk.lock();
                if (++done == parts) done_cv.notify_all();
            }
        }
    }
    // f(0..parts-1) on the pool plus the calling thread; returns when all are done
    void parallel(int nparts, const std::function<void(int)>& f) {
        std::unique_lock<std::mutex> lk(m);
        job = f;
        parts = nparts;
        next = 0;
        done = 0;
        gen++;
        cv.notify_all();
        while (next < parts) {
            const int k = next++;
            lk.unlock();
            f(k);
            lk.lock();
            if (++done == parts) done_cv.notify_all();
        }
        done_cv.wait(lk, [&] { return done == parts; });
        parts = 0;
    }
};

namespace {

constexpr size_t kHostPiece = 8u << 20;  // bytes per staged piece

// the two pinned staging pieces and their events
void free_staging(skml_ctx* c) {
    for (int b = 0; b < 2; b++) {
        if (c->hpin[b]) (void)hipHostFree(c->hpin[b]);
        if (c->hev[b]) (void)hipEventDestroy(c->hev[b]);
        c->hpin[b] = nullptr;
        c->hev[b] = nullptr;
    }
}

// the device copies of the host buffers grow in whole MiB
int ensure_dev_buf(skml_ctx* c, DevBuf& b, size_t bytes) {
    return reserve(c, b, bytes, align_up(bytes, 1u << 20), "device buffer");
}

int ensure_host_path(skml_ctx* c) {
    if (!c->hpin[0] || !c->hpin[1] || !c->hev[0] || !c->hev[1]) {
        // all four or nothing: a partial setup is freed so the next call starts over
        auto undo = [c]() {
            free_staging(c);
            (void)hipGetLastError();
        };
        undo();
        for (int b = 0; b < 2; b++) {
            if (hipHostMalloc(&c->hpin[b], kHostPiece, hipHostMallocDefault) != hipSuccess) {
                c->hpin[b] = nullptr;
                undo();
                return fail(SKML_E_OOM, "pinned staging of %zu B", kHostPiece);
            }
            if (hipEventCreateWithFlags(&c->hev[b], hipEventDisableTiming) != hipSuccess) {
                c->hev[b] = nullptr;
                undo();
                return fail(SKML_E_HIP, "staging event");
            }
        }
    }
    if (!c->pool) {
        int n = 4;  // host copy threads besides the caller (SKML_HOST_THREADS overrides)
        if (const char* e = std::getenv("SKML_HOST_THREADS")) n = std::max(0, std::min(64, std::atoi(e)));
        c->pool = new CopyPool(n);
    }
    return SKML_OK;
}

// memcpy on the pool, split into cache-friendly slices
void pool_copy(skml_ctx* c, void* dst, const void* src, size_t bytes) {
    const size_t slice = 1u << 20;
    const int parts = (int)((bytes + slice - 1) / slice);
    if (parts <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    c->pool->parallel(parts, [&](int k) {
        const size_t o = (size_t)k * slice, len = std::min(slice, bytes - o);
        std::memcpy((char*)dst + o, (const char*)src + o, len);
    });
}

bool is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // a plain pageable pointer: not an error for us
        return false;
    }
    return a.type == hipMemoryTypeHost && a.hostPointer != nullptr;
}

// host -> device, staged through the pinned pair unless the source is pinned itself
int upload(skml_ctx* c, void* dev, const void* host, size_t bytes) {
    if (!bytes) return SKML_OK;
    if (is_pinned(host)) {
        HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
        return SKML_OK;
    }
    size_t off = 0;
    for (int i = 0; off < bytes; i++) {
        const int b = i & 1;
        const size_t len = std::min(kHostPiece, bytes - off);
        // the DMA out of buffer b (this call's piece i-2, or an earlier call's last pieces) is done
        HIP_TRY(hipEventSynchronize(c->hev[b]));
        pool_copy(c, c->hpin[b], (const char*)host + off, len);
        HIP_TRY(hipMemcpyAsync((char*)dev + off, c->hpin[b], len, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->hev[b], c->stream));
        off += len;
    }
    return SKML_OK;
}

// device -> host (synchronous: returns with the bytes in `host`)
int download(skml_ctx* c, void* host, const void* dev, size_t bytes) {
    if (!bytes) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SKML_OK;
    }
    if (is_pinned(host)) {
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SKML_OK;
    }
    const size_t pieces = (bytes + kHostPiece - 1) / kHostPiece;
    auto issue = [&](size_t i) -> int {
        const int b = (int)(i & 1);
        const size_t off = i * kHostPiece, len = std::min(kHostPiece, bytes - off);
        HIP_TRY(hipMemcpyAsync(c->hpin[b], (const char*)dev + off, len, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->hev[b], c->stream));
        return SKML_OK;
    };
    int st = issue(0);
    if (!st && pieces > 1) st = issue(1);
    for (size_t i = 0; i < pieces && !st; i++) {
        const int b = (int)(i & 1);
        const size_t off = i * kHostPiece, len = std::min(kHostPiece, bytes - off);
        HIP_TRY(hipEventSynchronize(c->hev[b]));
        pool_copy(c, (char*)host + off, c->hpin[b], len);
        if (i + 2 < pieces) st = issue(i + 2);
    }
    return st;
}

}  // namespace

void skml::destroy_host_path(skml_ctx* c) {
    delete c->pool;
    c->pool = nullptr;
    free_staging(c);
    for (DevBuf* b : {&c->hx, &c->hp, &c->hk}) release(*b);
}

extern "C" {

int skml_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(SKML_E_ARG, "out is NULL");
    *out = nullptr;
    if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SKML_E_OOM, "pinned host allocation of %zu B", bytes);
    }
    return SKML_OK;
}

int skml_host_free(void* p) {
    if (p) HIP_TRY(hipHostFree(p));
    return SKML_OK;
}

}  // extern "C"

namespace {

// the device payload written by an encode on device buffers -> bytes in use (header, splits, codes)
size_t payload_used(const skml_dense_header& h) {
    return (size_t)h.codes_offset + ((size_t)h.n * (size_t)h.code_bits + 7) / 8;
}

// A host payload's header, checked for self-consistency against its length.
int host_header(const void* payload, size_t len, skml_dense_header* h, bool need_ok = true) {
    if (!payload || len < sizeof(skml_dense_header)) return fail(SKML_E_ARG, "payload too short");
    std::memcpy(h, payload, sizeof(*h));
    if (h->magic != SKML_DENSE_MAGIC) return fail(SKML_E_STATE, "not a dense payload");
    if (need_ok && h->status == SKML_E_NAN) return fail(SKML_E_NAN, "Encounter NaN value");
    if (need_ok && h->status != SKML_OK) return fail(SKML_E_STATE, "payload status %d", h->status);
    if (h->n < 0 || h->n > 0x7FFFFFFFLL || h->bin_num < 2 || h->bin_num > h->req_bins || h->req_bins > SKML_MAX_BINS ||
        h->code_bits != code_bits_for(h->bin_num) || h->codes_offset != (int64_t)dense_codes_offset(h->req_bins) ||
        h->zero_idx < 0 || h->zero_idx >= h->bin_num)
        return fail(SKML_E_ARG, "inconsistent payload header");
    if (h->status == SKML_OK && len < payload_used(*h))
        return fail(SKML_E_ARG, "payload of %zu B, header needs %zu", len, payload_used(*h));
    return SKML_OK;
}

template <typename T, typename Encode>
int encode_host(skml_ctx* c, const T* x, int64_t n, const skml_params* p, void* payload, size_t cap, size_t* written,
                Encode encode) {
    skml_params def;
    p = params_or_default(p, &def, /*clear_dedup=*/false);
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (n < 0 || n > 0x7FFFFFFFLL) return fail(SKML_E_ARG, "n=%lld outside Java int range", (long long)n);
    if (p->bin_num < 2 || p->bin_num > SKML_MAX_BINS) return fail(SKML_E_ARG, "Invalid partition number: %d", p->bin_num);
    const size_t nb = skml_dense_payload_bytes(n, p->bin_num);
    if (!payload) {  // size query: an upper bound of the bytes written
        if (written) *written = nb;
        return SKML_OK;
    }
    if (n > 0 && !x) return fail(SKML_E_ARG, "x is NULL");
    HIP_TRY(hipSetDevice(c->device));
    int st;
    if ((st = ensure_host_path(c))) return st;
    if ((st = ensure_dev_buf(c, c->hx, std::max<size_t>(16, sizeof(T) * (size_t)n)))) return st;
    if ((st = ensure_dev_buf(c, c->hp, nb))) return st;
    if ((st = upload(c, c->hx.p, x, sizeof(T) * (size_t)n))) return st;
    if ((st = encode(c, (const T*)c->hx.p, n, p, c->hp.p, c->hp.cap))) return st;
    skml_dense_header h;
    HIP_TRY(hipMemcpyAsync(&h, c->hp.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h.status == SKML_E_NAN) return fail(SKML_E_NAN, "Encounter NaN value");
    const size_t used = payload_used(h);
    if (written) *written = used;
    if (cap < used) return fail(SKML_E_ARG, "payload capacity %zu < %zu", cap, used);
    return download(c, payload, c->hp.p, used);
}

template <typename T, typename Decode>
int decode_host(skml_ctx* c, const void* payload, size_t len, T* out, int64_t n, Decode decode) {
    if (!c || (n > 0 && !out)) return fail(SKML_E_ARG, "bad arguments");
    skml_dense_header h;
    int st = host_header(payload, len, &h);
    if (st) return st;
    if (h.n != n) return fail(SKML_E_ARG, "payload holds %lld values, asked for %lld", (long long)h.n, (long long)n);
    HIP_TRY(hipSetDevice(c->device));
    if ((st = ensure_host_path(c))) return st;
    if ((st = ensure_dev_buf(c, c->hp, skml_dense_payload_bytes(n, h.req_bins)))) return st;
    if ((st = ensure_dev_buf(c, c->hx, std::max<size_t>(16, sizeof(T) * (size_t)n)))) return st;
    if ((st = upload(c, c->hp.p, payload, payload_used(h)))) return st;
    if ((st = decode(c, c->hp.p, (T*)c->hx.p, n))) return st;
    return download(c, out, c->hx.p, sizeof(T) * (size_t)n);
}

}  // namespace

extern "C" {

// params->quant_type = SKML_UNIFORM selects UniformQuantizer (Quantizer.newQuantizer's switch,
// base/Quantizer.java:126-136, as on the sparse path); otherwise params->parallelism > 1 selects
// QuantileQuantizer.parallelQuantize with that many slices, else quantize.
int skml_dense_encode_host_f32(skml_ctx* c, const float* x, int64_t n, const skml_params* p, void* payload,
                               size_t cap, size_t* written) {
    return encode_host<float>(c, x, n, p, payload, cap, written,
                              [](skml_ctx* c2, const float* xd, int64_t m, const skml_params* q, void* pl, size_t cp) {
                                  return q->quant_type == SKML_UNIFORM ? skml_dense_encode_uniform_f32(c2, xd, m, q, pl, cp)
                                         : q->parallelism > 1
                                             ? skml_dense_encode_parallel_f32(c2, xd, m, q->parallelism, q, pl, cp)
                                             : skml_dense_encode_f32(c2, xd, m, q, pl, cp);
                              });
}

int skml_dense_encode_host_f64(skml_ctx* c, const double* x, int64_t n, const skml_params* p, void* payload,
                               size_t cap, size_t* written) {
    return encode_host<double>(c, x, n, p, payload, cap, written,
                               [](skml_ctx* c2, const double* xd, int64_t m, const skml_params* q, void* pl, size_t cp) {
                                   return q->quant_type == SKML_UNIFORM ? skml_dense_encode_uniform_f64(c2, xd, m, q, pl, cp)
                                          : q->parallelism > 1
                                              ? skml_dense_encode_parallel_f64(c2, xd, m, q->parallelism, q, pl, cp)
                                              : skml_dense_encode_f64(c2, xd, m, q, pl, cp);
                               });
}

int skml_dense_decode_host_f32(skml_ctx* c, const void* payload, size_t len, float* out, int64_t n) {
    return decode_host<float>(c, payload, len, out, n, skml_dense_decode_f32);
}

int skml_dense_decode_host_f64(skml_ctx* c, const void* payload, size_t len, double* out, int64_t n) {
    return decode_host<double>(c, payload, len, out, n, skml_dense_decode_f64);
}

int skml_dense_info_host(const void* payload, size_t len, skml_dense_header* hdr, double* splits, int32_t cap) {
    if (!hdr) return fail(SKML_E_ARG, "hdr is NULL");
    int st = host_header(payload, len, hdr, false);
    if (st) return st;
    if (hdr->status == SKML_E_NAN) return fail(SKML_E_NAN, "Encounter NaN value");
    if (splits) {
        const int ns = hdr->bin_num - 1;
        if (ns > cap) return fail(SKML_E_ARG, "splits capacity %d < %d", cap, ns);
        std::memcpy(splits, (const char*)payload + kHeaderBytes, sizeof(double) * (size_t)ns);
    }
    return hdr->status;
}

int skml_dense_bins_host(const void* payload, size_t len, int32_t* bins, int64_t n) {
    skml_dense_header h;
    int st = host_header(payload, len, &h);
    if (st) return st;
    if (h.n != n || (n > 0 && !bins)) return fail(SKML_E_ARG, "bins of %lld values, payload holds %lld", (long long)n,
                                                  (long long)h.n);
    const uint8_t* codes = (const uint8_t*)payload + h.codes_offset;
    const int b = h.code_bits;
    for (int64_t e = 0; e < n; e++) {  // LSB-first packed codes (include/skml.h)
        const uint64_t bit = (uint64_t)e * (uint64_t)b;
        uint32_t v;
        if (b == 16) v = (uint32_t)codes[2 * e] | ((uint32_t)codes[2 * e + 1] << 8);
        else v = (codes[bit >> 3] >> (bit & 7)) & ((1u << b) - 1u);
        bins[e] = (int32_t)v;
    }
    return SKML_OK;
}

int skml_dense_times_by_host(void* payload, size_t len, double x) {
    skml_dense_header h;
    int st = host_header(payload, len, &h);
    if (st) return st;
    double* sp = reinterpret_cast<double*>((char*)payload + kHeaderBytes);  // Quantizer.timesBy (:119-124)
    for (int i = 0; i < h.bin_num - 1; i++) sp[i] *= x;
    h.min *= x;
    h.max *= x;
    std::memcpy(payload, &h, sizeof(h));
    return SKML_OK;
}

int skml_sparse_encode_kv_host_f32(skml_ctx* c, const int32_t* keys, const float* vals, int64_t nnz,
                                   const skml_params* p, skml_sparse** out) {
    if (!c || !out || nnz < 0 || (nnz > 0 && (!keys || !vals))) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    int st;
    const size_t bytes = std::max<size_t>(16, 4 * (size_t)nnz);
    if ((st = ensure_host_path(c))) return st;
    if ((st = ensure_dev_buf(c, c->hx, bytes))) return st;
    if ((st = ensure_dev_buf(c, c->hk, bytes))) return st;
    if ((st = upload(c, c->hk.p, keys, 4 * (size_t)nnz))) return st;
    if ((st = upload(c, c->hx.p, vals, 4 * (size_t)nnz))) return st;
    return skml_sparse_encode_kv_f32(c, (const int32_t*)c->hk.p, (const float*)c->hx.p, nnz, p, out);
}

int skml_sparse_encode_kv_host_f64(skml_ctx* c, const int32_t* keys, const double* vals, int64_t nnz,
                                   const skml_params* p, skml_sparse** out) {
    if (!c || !out || nnz < 0 || (nnz > 0 && (!keys || !vals))) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    int st;
    if ((st = ensure_host_path(c))) return st;
    if ((st = ensure_dev_buf(c, c->hx, std::max<size_t>(16, 8 * (size_t)nnz)))) return st;
    if ((st = ensure_dev_buf(c, c->hk, std::max<size_t>(16, 4 * (size_t)nnz)))) return st;
    if ((st = upload(c, c->hk.p, keys, 4 * (size_t)nnz))) return st;
    if ((st = upload(c, c->hx.p, vals, 8 * (size_t)nnz))) return st;
    return skml_sparse_encode_kv_f64(c, (const int32_t*)c->hk.p, (const double*)c->hx.p, nnz, p, out);
}

}  // extern "C"

namespace {
template <typename T, typename Dec>
int sparse_decode_host(skml_ctx* c, const skml_sparse* s, int32_t* keys, T* vals, Dec dec) {
    int64_t n = 0;
    if (!c || !s || skml_sparse_nnz(s, &n)) return fail(SKML_E_ARG, "bad arguments");
    if (n > 0 && (!keys || !vals)) return fail(SKML_E_ARG, "keys/vals are NULL");
    HIP_TRY(hipSetDevice(c->device));
    int st;
    if ((st = ensure_host_path(c))) return st;
    if ((st = ensure_dev_buf(c, c->hx, std::max<size_t>(16, sizeof(T) * (size_t)n)))) return st;
    if ((st = ensure_dev_buf(c, c->hk, std::max<size_t>(16, 4 * (size_t)n)))) return st;
    if ((st = dec(c, s, (int32_t*)c->hk.p, (T*)c->hx.p))) return st;
    if ((st = download(c, keys, c->hk.p, 4 * (size_t)n))) return st;
    return download(c, vals, c->hx.p, sizeof(T) * (size_t)n);
}
}  // namespace

extern "C" {

int skml_sparse_decode_host_f32(skml_ctx* c, const skml_sparse* s, int32_t* keys, float* vals) {
    return sparse_decode_host<float>(c, s, keys, vals, skml_sparse_decode_f32);
}

int skml_sparse_decode_host_f64(skml_ctx* c, const skml_sparse* s, int32_t* keys, double* vals) {
    return sparse_decode_host<double>(c, s, keys, vals, skml_sparse_decode_f64);
}

int skml_delta_encode_host(skml_ctx* c, const int32_t* keys, int64_t n, int32_t* num_intervals, int32_t* flag_kind,
                           int64_t* n_flag_bits, int64_t* n_delta_bits, uint64_t* flag_words, uint64_t* delta_words,
                           int64_t words_cap) {
    if (!c || n <= 0 || !keys) return fail(SKML_E_ARG, "bad delta arguments");
    HIP_TRY(hipSetDevice(c->device));
    int st;
    if ((st = ensure_host_path(c))) return st;
    // a stream never exceeds 33 bits per key (16-bit flags are at most 4 bits, deltas at most 32)
    const size_t wcap = ((size_t)n * 33 + 63) / 64 + 1;
    if ((st = ensure_dev_buf(c, c->hk, 4 * (size_t)n))) return st;
    if ((st = ensure_dev_buf(c, c->hx, 8 * wcap))) return st;
    if ((st = ensure_dev_buf(c, c->hp, 8 * wcap))) return st;
    if ((st = upload(c, c->hk.p, keys, 4 * (size_t)n))) return st;
    int64_t nfb = 0, ndb = 0;
    if ((st = skml_delta_encode(c, (const int32_t*)c->hk.p, n, num_intervals, flag_kind, &nfb, &ndb, (uint64_t*)c->hx.p,
                                (uint64_t*)c->hp.p, (int64_t)wcap)))
        return st;
    if (n_flag_bits) *n_flag_bits = nfb;
    if (n_delta_bits) *n_delta_bits = ndb;
    const int64_t fw = (nfb + 63) / 64, dw = (ndb + 63) / 64;
    if (!flag_words && !delta_words) return SKML_OK;
    if (fw > words_cap || dw > words_cap)
        return fail(SKML_E_ARG, "words_cap %lld < needed %lld", (long long)words_cap, (long long)std::max(fw, dw));
    if (flag_words && (st = download(c, flag_words, c->hx.p, 8 * (size_t)fw))) return st;
    if (delta_words && (st = download(c, delta_words, c->hp.p, 8 * (size_t)dw))) return st;
    return SKML_OK;
}

int skml_delta_decode_host(skml_ctx* c, int64_t n, int32_t num_intervals, int32_t flag_kind, const uint64_t* flag_words,
                           int64_t n_flag_words, const uint64_t* delta_words, int64_t n_delta_words, int32_t* keys) {
    if (!c || n <= 0 || !keys || n_flag_words < 0 || n_delta_words < 0 || (n_flag_words && !flag_words) ||
        (n_delta_words && !delta_words))
        return fail(SKML_E_ARG, "bad delta decode arguments");
    HIP_TRY(hipSetDevice(c->device));
    int st;
    if ((st = ensure_host_path(c))) return st;
    // zero words past the trimmed streams (BitSet.toLongArray drops trailing zero words)
    const size_t fpad = 8 * ((size_t)n_flag_words + 64), dpad = 8 * ((size_t)n_delta_words + 64);
    if ((st = ensure_dev_buf(c, c->hx, fpad))) return st;
    if ((st = ensure_dev_buf(c, c->hp, dpad))) return st;
    if ((st = ensure_dev_buf(c, c->hk, 4 * (size_t)n))) return st;
    HIP_TRY(hipMemsetAsync(c->hx.p, 0, fpad, c->stream));
    HIP_TRY(hipMemsetAsync(c->hp.p, 0, dpad, c->stream));
    if ((st = upload(c, c->hx.p, flag_words, 8 * (size_t)n_flag_words))) return st;
    if ((st = upload(c, c->hp.p, delta_words, 8 * (size_t)n_delta_words))) return st;
    if ((st = skml_delta_decode(c, n, num_intervals, flag_kind, (const uint64_t*)c->hx.p, n_flag_words,
                                (const uint64_t*)c->hp.p, n_delta_words, (int32_t*)c->hk.p)))
        return st;
    return download(c, keys, c->hk.p, 4 * (size_t)n);
}

}  // extern "C"
