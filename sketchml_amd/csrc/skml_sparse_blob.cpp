// skml_sparse_blob.cpp -- the exchange form of a sparse payload (include/skml.h, "Sparse path"):
// one contiguous device blob per payload (SpBlobHeader, skml_sparse.h), its export and import,
// and Gradient.sum over gathered blobs.
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "skml_sparse_host.hpp"

using namespace skml;

namespace {
struct BlobLayout {
    size_t off_groups, off_quant, off_values, off_tables, off_flags, off_deltas, total;
    int32_t quant_bytes;
    int table_width;  // the MinMax cells: the payload's exact narrow image (8 / 16 bits) when it has one
};
BlobLayout blob_layout(const skml_sparse* s) {
    BlobLayout L;
    L.quant_bytes = (int32_t)(kHeaderBytes + sizeof(double) * (size_t)std::max(s->hdr.bin_num - 1, 0));
    L.table_width = s->tnar ? s->tnar_width : 32;
    L.off_groups = 256;
    L.off_quant = L.off_groups + align_up(sizeof(SpGroups), 256);
    L.off_values = L.off_quant + align_up((size_t)L.quant_bytes, 256);
    L.off_tables = L.off_values + align_up(sizeof(double) * std::max<size_t>(s->qvalues.size(), 1), 256);
    L.off_flags = L.off_tables + align_up((size_t)L.table_width / 8 * (size_t)std::max<int64_t>(s->ncells, 1), 256);
    L.off_deltas = L.off_flags + align_up(sizeof(uint64_t) * (size_t)s->n_flag_words, 256);
    L.total = L.off_deltas + align_up(sizeof(uint64_t) * (size_t)s->n_delta_words, 256);
    return L;
}

// A blob's group table, checked for the invariants the decode kernels index by (a corrupt or
// foreign blob must fail here, not fault on the device).
int check_blob_groups(const SpBlobHeader& h, const SpGroups& G) {
    auto bad = [](const char* what) { return fail(SKML_E_ARG, "sparse blob: inconsistent %s", what); };
    if (G.G < 1 || G.G > kMaxGroups || G.rows < 0 || G.rows > kMaxRows) return bad("group / row count");
    if (G.bin_num < 1 || G.bin_num > h.nvalues || G.zero < 0 || G.zero >= G.bin_num) return bad("bins");
    if (h.version >= 2 && h.table_width != 32 && h.table_width != tnar_width_for(G.bin_num)) return bad("cell width");
    if (G.gstart[0] != 0 || G.gstart[G.G] != h.nnz || G.fb[0] != 0 || G.db[0] != 0) return bad("stream starts");
    if (G.fb[G.G] != h.flag_bits || G.db[G.G] != h.delta_bits || G.ncells != h.ncells) return bad("stream totals");
    if (h.n_flag_words < (h.flag_bits + 63) / 64 + 1 || h.n_delta_words < (h.delta_bits + 63) / 64 + 1)
        return bad("word counts");
    int32_t k1 = 0;
    for (int g = 0; g < G.G; g++) {
        if (G.gstart[g + 1] < G.gstart[g] || G.fb[g + 1] < G.fb[g] || G.db[g + 1] < G.db[g]) return bad("offsets");
        const int64_t size = G.gstart[g + 1] - G.gstart[g];
        const int32_t m = G.m[g];
        if (m != 1 && m != 2 && m != 4 && m != 8 && m != 16) return bad("numIntervals");
        if (G.kind[g] != 0 && G.kind[g] != 1) return bad("flagKind");
        if (G.kind1_before[g] != k1) return bad("unary counts");
        if (G.kind[g]) k1 += (int32_t)size;
        if (size == 0) continue;
        if (G.cols[g] < 1 || G.tab_off[g] < 0 || G.tab_off[g] + (int64_t)G.rows * G.cols[g] > G.ncells)
            return bad("table shape");
        if (G.inv_cols[g] != 1.0 / (double)G.cols[g]) return bad("column reciprocal");
        for (int r = 0; r < G.rows; r++)
            if (G.hash_ids[g][r] < 0 || G.hash_ids[g][r] > 7) return bad("hash id");
    }
    return SKML_OK;
}

// A blob's header, checked against the `len` bytes it may span.
int blob_table_width(const SpBlobHeader* h) { return h->version >= 2 ? h->table_width : 32; }
int blob_check_header(const SpBlobHeader* h, size_t len) {
    if (h->magic != kSpBlobMagic || h->version < 1 || h->version > 2) return fail(SKML_E_STATE, "not a sparse blob");
    const int tw = blob_table_width(h);
    if (tw != 8 && tw != 16 && tw != 32) return fail(SKML_E_ARG, "sparse blob: cell width %d", tw);
    if (h->total_bytes < 256 || (size_t)h->total_bytes > len || h->nnz < 0 || h->nnz > INT32_MAX || h->ncells < 0 ||
        h->nvalues < 1 || h->nvalues > SKML_MAX_BINS || h->quant_bytes < kHeaderBytes ||
        h->off_groups != 256 || h->off_quant < h->off_groups + (int64_t)sizeof(SpGroups) ||
        h->off_values < h->off_quant + h->quant_bytes || h->off_tables < h->off_values + 8 * (int64_t)h->nvalues ||
        h->off_flags < h->off_tables + tw / 8 * h->ncells || h->off_deltas < h->off_flags + 8 * h->n_flag_words ||
        h->total_bytes < h->off_deltas + 8 * h->n_delta_words || (h->off_tables | h->off_flags | h->off_deltas) & 255)
        return fail(SKML_E_ARG, "sparse blob: inconsistent section offsets");
    return SKML_OK;
}

// A non-owning skml_sparse view of the blob at `dev`, from its host meta `meta` (header, group
// table, quantizer header + splits, values: the blob's bytes up to off_tables).
int blob_view(skml_ctx* c, const uint8_t* dev, const SpBlobHeader& h, const uint8_t* meta, skml_sparse* view) {
    std::memcpy(&view->g, meta + h.off_groups, sizeof(SpGroups));
    if (int e = check_blob_groups(h, view->g)) return e;
    std::memcpy(&view->hdr, meta + h.off_quant, sizeof(skml_dense_header));
    const double* sp = reinterpret_cast<const double*>(meta + h.off_quant + kHeaderBytes);
    const int ns = (h.quant_bytes - kHeaderBytes) / 8;
    view->splits.assign(sp, sp + ns);
    const double* qv = reinterpret_cast<const double*>(meta + h.off_values);
    view->qvalues.assign(qv, qv + h.nvalues);
    view->device = c->device;
    view->nnz = h.nnz;
    view->params = h.params;
    view->ncells = h.ncells;
    view->flag_bits = h.flag_bits;
    view->delta_bits = h.delta_bits;
    view->n_flag_words = h.n_flag_words;
    view->n_delta_words = h.n_delta_words;
    view->g_dev = reinterpret_cast<SpGroups*>(const_cast<uint8_t*>(dev) + h.off_groups);
    uint8_t* tab = const_cast<uint8_t*>(dev) + h.off_tables;
    const int tw = blob_table_width(&h);
    view->tables = tw == 32 ? reinterpret_cast<int32_t*>(tab) : nullptr;
    view->tnar = tw == 32 ? nullptr : tab;
    view->tnar_width = tw == 32 ? 0 : tw;
    view->flag_words = reinterpret_cast<uint64_t*>(const_cast<uint8_t*>(dev) + h.off_flags);
    view->delta_words = reinterpret_cast<uint64_t*>(const_cast<uint8_t*>(dev) + h.off_deltas);
    return SKML_OK;
}

// The host meta of P blobs at `dev` + p * stride and their views: the first 16 KB of every blob
// (header, group table, quantizer and values of up to ~1,000 bins) in one strided device-to-host
// copy, and only if some blob's meta runs past that, every blob's meta in a second (a read-back
// per blob and section cost ~20 us of host round trip each, 16 of them for 8 payloads).
int blob_metas(skml_ctx* c, const uint8_t* dev, int P, size_t stride, SpBlobHeader* hs, skml_sparse* views) {
    if (!dev || P < 1 || stride < 256 || (stride & 255) || (reinterpret_cast<uintptr_t>(dev) & 255))
        return fail(SKML_E_ARG, "sparse blob: NULL, shorter than its header or not 256-byte aligned");
    hipStream_t st = c->stream;
    size_t w = std::min<size_t>(stride, 16384);
    uint8_t* pin = static_cast<uint8_t*>(ctx_pinned(c, w * (size_t)P));
    if (!pin) return fail(SKML_E_OOM, "pinned staging of %zu bytes", w * (size_t)P);
    HIP_TRY(hipMemcpy2DAsync(pin, w, dev, stride, w, (size_t)P, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    size_t meta_max = 0;
    for (int p = 0; p < P; p++) {
        std::memcpy(&hs[p], pin + (size_t)p * w, sizeof(SpBlobHeader));
        if (int e = blob_check_header(&hs[p], stride)) return fail(e, "payload %d: %s", p, skml_last_error());
        meta_max = std::max(meta_max, (size_t)hs[p].off_tables);
    }
    if (meta_max > w) {  // off_tables is a multiple of 256 below total_bytes <= stride
        w = meta_max;
        pin = static_cast<uint8_t*>(ctx_pinned(c, w * (size_t)P));
        if (!pin) return fail(SKML_E_OOM, "pinned staging of %zu bytes", w * (size_t)P);
        HIP_TRY(hipMemcpy2DAsync(pin, w, dev, stride, w, (size_t)P, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (int p = 0; p < P; p++)
        if (int e = blob_view(c, dev + (size_t)p * stride, hs[p], pin + (size_t)p * w, &views[p]))
            return fail(e, "payload %d: %s", p, skml_last_error());
    return SKML_OK;
}

// The host meta of a blob at `dev` (header, group table, quantizer header + splits, values) and a
// non-owning skml_sparse view of its device sections.
int blob_meta(skml_ctx* c, const uint8_t* dev, size_t len, SpBlobHeader* h, skml_sparse* view) {
    if (!dev || len < 256 || (reinterpret_cast<uintptr_t>(dev) & 255))
        return fail(SKML_E_ARG, "sparse blob: NULL, shorter than its header or not 256-byte aligned");
    if (int e = sync_to_host(c, h, dev, sizeof(*h))) return e;
    if (int e = blob_check_header(h, len)) return e;
    std::vector<uint8_t> meta((size_t)h->off_tables);
    if (int e = sync_to_host(c, meta.data(), dev, meta.size())) return e;
    return blob_view(c, dev, *h, meta.data(), view);
}

// a view points into memory it does not own: cleared before it goes out of scope, so no later
// change to skml_sparse's destruction can free the caller's blob
struct ViewGuard {
    skml_sparse* v;
    ~ViewGuard() {
        v->g_dev = nullptr;
        v->tables = nullptr;
        v->tnar = nullptr;
        v->flag_words = v->delta_words = nullptr;
        v->qpayload = nullptr;
    }
};
}  // namespace

extern "C" {

int skml_sparse_export_bytes(const skml_sparse* s, size_t* bytes) {
    if (!s || !bytes) return fail(SKML_E_ARG, "NULL argument");
    *bytes = blob_layout(s).total;
    return SKML_OK;
}

int skml_sparse_export(skml_ctx* c, const skml_sparse* s, void* dst, size_t cap) {
    if (!c || !s || !dst || (reinterpret_cast<uintptr_t>(dst) & 255)) return fail(SKML_E_ARG, "bad export arguments");
    const BlobLayout L = blob_layout(s);
    if (cap < L.total) return fail(SKML_E_ARG, "export capacity %zu < %zu", cap, L.total);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // the host-side sections go through the context's pinned staging in one copy
    const size_t host_bytes = L.off_tables;
    uint8_t* pin = static_cast<uint8_t*>(ctx_pinned(c, host_bytes));
    if (!pin) return fail(SKML_E_OOM, "pinned staging");
    HIP_TRY(hipStreamSynchronize(st));  // the staging buffer may still feed an earlier copy
    std::memset(pin, 0, host_bytes);
    SpBlobHeader h{};
    h.magic = kSpBlobMagic;
    h.version = 2;
    h.table_width = L.table_width;
    h.total_bytes = (int64_t)L.total;
    h.nnz = s->nnz;
    h.ncells = s->ncells;
    h.n_flag_words = s->n_flag_words;
    h.n_delta_words = s->n_delta_words;
    h.flag_bits = s->flag_bits;
    h.delta_bits = s->delta_bits;
    h.nvalues = (int32_t)s->qvalues.size();
    h.quant_bytes = L.quant_bytes;
    h.off_groups = (int64_t)L.off_groups;
    h.off_quant = (int64_t)L.off_quant;
    h.off_values = (int64_t)L.off_values;
    h.off_tables = (int64_t)L.off_tables;
    h.off_flags = (int64_t)L.off_flags;
    h.off_deltas = (int64_t)L.off_deltas;
    h.params = s->params;
    std::memcpy(pin, &h, sizeof(h));
    SpGroups g = s->g;
    for (int k = 0; k < kMaxGroups; k++) g.inv_cols[k] = g.cols[k] > 0 ? 1.0 / (double)g.cols[k] : 0.0;
    std::memcpy(pin + L.off_groups, &g, sizeof(g));
    std::memcpy(pin + L.off_quant, &s->hdr, sizeof(skml_dense_header));
    if (!s->splits.empty())
        std::memcpy(pin + L.off_quant + kHeaderBytes, s->splits.data(), sizeof(double) * s->splits.size());
    if (!s->qvalues.empty()) std::memcpy(pin + L.off_values, s->qvalues.data(), sizeof(double) * s->qvalues.size());
    uint8_t* d = static_cast<uint8_t*>(dst);
    HIP_TRY(hipMemcpyAsync(d, pin, host_bytes, hipMemcpyHostToDevice, st));
    if (s->ncells > 0)  // the exact narrow image when the payload has one, else the int32 cells
        HIP_TRY(hipMemcpyAsync(d + L.off_tables, s->tnar ? s->tnar : static_cast<const void*>(s->tables),
                               (size_t)L.table_width / 8 * (size_t)s->ncells, hipMemcpyDeviceToDevice, st));
    if (s->n_flag_words > 0)
        HIP_TRY(hipMemcpyAsync(d + L.off_flags, s->flag_words, sizeof(uint64_t) * (size_t)s->n_flag_words,
                               hipMemcpyDeviceToDevice, st));
    if (s->n_delta_words > 0)
        HIP_TRY(hipMemcpyAsync(d + L.off_deltas, s->delta_words, sizeof(uint64_t) * (size_t)s->n_delta_words,
                               hipMemcpyDeviceToDevice, st));
    // the copies read the payload's block: they complete before the call returns, so a payload
    // freed right after its export hands the pool a block with no pending reader (BlockPool)
    HIP_TRY(hipStreamSynchronize(st));
    return SKML_OK;
}

int skml_sparse_import(skml_ctx* c, const void* blob, size_t len, skml_sparse** out) {
    if (!c || !out) return fail(SKML_E_ARG, "bad import arguments");
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    SpBlobHeader h;
    skml_sparse view;
    ViewGuard vg{&view};
    if (int e = blob_meta(c, static_cast<const uint8_t*>(blob), len, &h, &view)) return e;
    // an owned copy: the caller's gathered buffer may be reused by the next exchange
    skml_sparse* s = new skml_sparse();
    PayloadOwner own(s, st);
    s->device = view.device;
    s->nnz = view.nnz;
    s->params = view.params;
    s->hdr = view.hdr;
    s->splits = view.splits;
    s->qvalues = view.qvalues;
    s->g = view.g;
    s->ncells = view.ncells;
    s->flag_bits = view.flag_bits;
    s->delta_bits = view.delta_bits;
    s->n_flag_words = view.n_flag_words;
    s->n_delta_words = view.n_delta_words;
    // a narrow blob keeps its exact image (the restore gathers from it) and gets its int32 cells
    // back (serialisation, group info)
    const int tw = view.tnar ? view.tnar_width : 0;
    const size_t o_tab = align_up(sizeof(SpGroups), 256);
    const size_t o_tn = o_tab + align_up(sizeof(int32_t) * (size_t)std::max<int64_t>(s->ncells, 1), 256);
    const size_t o_fw = o_tn + (tw ? align_up((size_t)tw / 8 * (size_t)std::max<int64_t>(s->ncells, 1), 256) : 0);
    const size_t o_dw = o_fw + align_up(sizeof(uint64_t) * (size_t)s->n_flag_words, 256);
    const size_t o_qv = o_dw + align_up(sizeof(uint64_t) * (size_t)s->n_delta_words, 256);
    const size_t total = o_qv + sizeof(double) * std::max<size_t>(s->qvalues.size(), 1);
    char* blk = static_cast<char*>(block_get(s->device, total, &s->block_cap));
    if (!blk) return fail(SKML_E_OOM, "imported sparse payload of %zu bytes", total);
    s->qv_dev = reinterpret_cast<double*>(blk + o_qv);
    s->block = blk;
    s->g_dev = reinterpret_cast<SpGroups*>(blk);
    s->tables = reinterpret_cast<int32_t*>(blk + o_tab);
    s->tnar = tw ? blk + o_tn : nullptr;
    s->tnar_width = tw;
    s->flag_words = reinterpret_cast<uint64_t*>(blk + o_fw);
    s->delta_words = reinterpret_cast<uint64_t*>(blk + o_dw);
    SP_TRY(hipMemcpyAsync(s->g_dev, view.g_dev, sizeof(SpGroups), hipMemcpyDeviceToDevice, st));
    if (!s->qvalues.empty())  // the blob's values section: the device copy of quantValues
        SP_TRY(hipMemcpyAsync(s->qv_dev, static_cast<const uint8_t*>(blob) + h.off_values,
                              sizeof(double) * s->qvalues.size(), hipMemcpyDeviceToDevice, st));
    s->qv_dev_ok = !s->qvalues.empty();
    if (s->ncells > 0 && tw) {
        SP_TRY(hipMemcpyAsync(s->tnar, view.tnar, (size_t)tw / 8 * (size_t)s->ncells, hipMemcpyDeviceToDevice, st));
        SP_TRY(launch_widen_cells(st, s->tnar, tw, s->ncells, s->g.fill, s->tables));
    } else if (s->ncells > 0) {
        SP_TRY(hipMemcpyAsync(s->tables, view.tables, sizeof(int32_t) * (size_t)s->ncells, hipMemcpyDeviceToDevice, st));
    }
    if (s->n_flag_words > 0)
        SP_TRY(hipMemcpyAsync(s->flag_words, view.flag_words, sizeof(uint64_t) * (size_t)s->n_flag_words,
                              hipMemcpyDeviceToDevice, st));
    if (s->n_delta_words > 0)
        SP_TRY(hipMemcpyAsync(s->delta_words, view.delta_words, sizeof(uint64_t) * (size_t)s->n_delta_words,
                              hipMemcpyDeviceToDevice, st));
    SP_TRY(hipStreamSynchronize(st));
    own.release(out);
    return SKML_OK;
}

}  // extern "C"

namespace {

// Gradient.sum over P exported sparse payloads (ml/gradient/Gradient.scala:44-49): out = +0.0,
// then for p = 0..P-1 in order DenseDoubleGradient.plusBy(payload p .toAuto)
// (DenseDoubleGradient.scala:38; SketchGradient.toSparse -> SparseDoubleGradient.toAuto), then
// out *= scale unless scale == 1.  A payload whose live count (|v| > 1e-8) exceeds dim * 2 / 3 (Java
// int arithmetic) reaches plusBy in dense form: only its live values are added, and every entry
// takes the dense form's + 0.0.  SketchGradient.toSparse builds a SparseDoubleGradient from the
// restored keys, whose constructor requires them strictly increasing and inside [0, dim)
// (SparseDoubleGradient.scala:9-14): a key repeated across a payload's groups, a run that does not
// ascend or a key out of range fails the whole sum with SKML_E_ARG.
// O: the type `out` is returned in.  The sum is in double whatever O is: a narrow O is written
// by the last tile launch alone, and the launches before it (more than 8 payloads in the wave-tile
// form, or more than one scratch batch) keep the sum in a `dim`-double accumulator of the context's
// scratch; the double entry continues in `out` itself.
inline hipError_t launch_agg_last(hipStream_t st, const AggPayload* pays, int P, int64_t ntiles, int64_t dim, float* out,
                                  const double* src, int from_out, double scale, unsigned* err, bool vt,
                                  const int32_t* kb, const uint8_t* bb, bool any_dense) {
    return launch_agg_tiles_f32(st, pays, P, ntiles, dim, out, src, from_out, scale, err, vt, kb, bb, any_dense);
}
inline hipError_t launch_agg_last(hipStream_t st, const AggPayload* pays, int P, int64_t ntiles, int64_t dim, bf16_t* out,
                                  const double* src, int from_out, double scale, unsigned* err, bool vt,
                                  const int32_t* kb, const uint8_t* bb, bool any_dense) {
    return launch_agg_tiles_bf16(st, pays, P, ntiles, dim, out, src, from_out, scale, err, vt, kb, bb, any_dense);
}
inline hipError_t launch_agg_last(hipStream_t st, const AggPayload* pays, int P, int64_t ntiles, int64_t dim, f16_t* out,
                                  const double* src, int from_out, double scale, unsigned* err, bool vt,
                                  const int32_t* kb, const uint8_t* bb, bool any_dense) {
    return launch_agg_tiles_f16(st, pays, P, ntiles, dim, out, src, from_out, scale, err, vt, kb, bb, any_dense);
}

template <typename O>
int decode_sum_any(skml_ctx* c, const void* blobs, int32_t P, size_t stride, int64_t dim, double scale, O* out) {
    if (!c || !blobs || P < 1 || dim < 0 || dim > (int64_t)INT32_MAX || (dim > 0 && !out) || stride % 256)
        return fail(SKML_E_ARG, "bad sparse decode_sum arguments (P >= 1, 256-byte stride, dim in Java int)");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<SpBlobHeader> hs((size_t)P);
    std::vector<skml_sparse> views((size_t)P);  // non-owning: skml_sparse frees nothing on destruction
    if (int e = blob_metas(c, static_cast<const uint8_t*>(blobs), P, stride, hs.data(), views.data())) return e;
    const int64_t lim = (int64_t)(int32_t)((uint32_t)dim * 2u) / 3;  // dim * 2 / 3 with Java int wrap
    // run bounds are taken per tile of the tile kernel: 512 keys for the wave-tile form, else 4,096
    const int64_t ntiles_max = sp_tiles(dim, (int64_t)1 << agg_tile_bits(true));
    auto bin_width = [&](int p) { return views[(size_t)p].qvalues.size() <= 256 ? 1 : 2; };
    // a payload's restored keys and bins, each 16-byte aligned in its scratch buffer
    auto key_words = [&](int p) { return (views[(size_t)p].nnz + 3) & ~int64_t{3}; };
    auto bin_bytes = [&](int p) { return (views[(size_t)p].nnz * bin_width(p) + 15) & ~int64_t{15}; };
    // payloads in batches whose restored keys + bins + run bounds fit the scratch budget; the first
    // batch starts the sum at +0.0, later ones continue from it, the last one applies the scale
    // (plan_sum_batches; kSumBudget unless the test hook skml_debug_sparse_sum_budget set a smaller one)
    t_sum_batches = t_sum_launches = 0;
    const int64_t hook = g_sum_budget.load();
    const size_t budget = hook > 0 ? std::min((size_t)hook, kSumBudget) : kSumBudget;
    auto need_of = [&](int p) {
        return (size_t)key_words(p) * 4 + (size_t)bin_bytes(p) +
               (size_t)views[(size_t)p].g.G * (size_t)(ntiles_max + 1) * 4 + 1024;
    };
    // SketchGradient.toSparse of an empty restore builds SparseDoubleGradient(dim, [], []), whose
    // constructor reads indices.head (SparseDoubleGradient.scala:11) and throws: so does the sum
    for (int p = 0; p < P; p++)
        if (views[(size_t)p].nnz == 0)
            return fail(SKML_E_ARG, "payload %d restores no keys: head of empty list (SparseDoubleGradient.scala:11)", p);
    std::vector<int> todo;
    for (int p = 0; p < P; p++) todo.push_back(p);
    uint8_t* small = scratch<uint8_t>(c, kSlotStatus, 1024 + sizeof(AggPayload) * (size_t)P);
    if (!small) return fail(SKML_E_OOM, "decode_sum scratch");
    unsigned* err = reinterpret_cast<unsigned*>(small);
    uint64_t* live = reinterpret_cast<uint64_t*>(small + 256);
    AggPayload* d_pays = reinterpret_cast<AggPayload*>(small + 1024);
    HIP_TRY(hipMemsetAsync(err, 0, sizeof(unsigned), st));
    std::vector<size_t> need;
    for (int p : todo) need.push_back(need_of(p));
    size_t at = 0;
    bool first = true;
    double* accd = nullptr;  // a narrow O: the sum between launches
    for (const size_t end : plan_sum_batches(need, budget)) {
        t_sum_batches++;
        int max_g = 0, max_nq = 0;
        for (size_t q = at; q < end; q++) {
            max_g = std::max(max_g, (int)views[(size_t)todo[q]].g.G);
            max_nq = std::max(max_nq, (int)views[(size_t)todo[q]].qvalues.size());
        }
        const bool vt = agg_vtiles_ok(max_g, max_nq);
        const int tile_bits = agg_tile_bits(vt);
        const int64_t ntiles = sp_tiles(dim, (int64_t)1 << tile_bits);
        int64_t nk = 0, nbb = 0, nb = 0;
        for (size_t q = at; q < end; q++) {
            nk += key_words(todo[q]);
            nbb += bin_bytes(todo[q]);
            nb += (int64_t)views[(size_t)todo[q]].g.G * (ntiles + 1);
        }
        int32_t* gk = scratch<int32_t>(c, kSlotCKeys, (size_t)nk);
        uint8_t* gbn = scratch<uint8_t>(c, kSlotCVals, (size_t)nbb);  // 1 or 2 bytes per bin
        int32_t* bounds = scratch<int32_t>(c, kSlotCells, (size_t)nb);
        if (!gk || !gbn || !bounds) return fail(SKML_E_OOM, "decode_sum scratch (%lld keys)", (long long)nk);
        HIP_TRY(hipMemsetAsync(bounds, 0, sizeof(int32_t) * (size_t)nb, st));  // empty groups: every bound 0
        // two lanes: payloads alternate between the caller's stream and the side context's (each
        // restore is a chain of small latency-bound kernels; two chains fill the chip better),
        // joined before the tiles; SKML_SERIAL, SKML_FORM_AGG_ONE_LANE or a single payload keep one
        skml_ctx* lanes[2] = {c, nullptr};
        hipStream_t side_st = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
        if (end - at > 1 && form(SKML_FORM_AGG_ONE_LANE) != 1 && ctx_side_fork(c, &side_st, &ev_fork, &ev_join) == SKML_OK) {
            lanes[1] = c->side;
            HIP_TRY(hipEventRecord(ev_fork, st));
            HIP_TRY(hipStreamWaitEvent(side_st, ev_fork, 0));
        }
        std::vector<AggPayload> pays;
        int64_t ko = 0, bbo = 0, bo = 0;
        for (size_t q = at; q < end; q++) {
            const int p = todo[q];
            const int li = lanes[1] && ((q - at) & 1) ? 1 : 0;
            skml_ctx* lc = lanes[li];
            hipStream_t ls = lc->stream;
            uint64_t* llive = live + li;
            const skml_sparse& v = views[(size_t)p];
            AggPayload a{};
            a.gk = gk + ko;
            a.nq = (int)v.qvalues.size();
            a.bw = bin_width(p);
            a.gb = gbn + bbo;
            a.qv = reinterpret_cast<const double*>(static_cast<const uint8_t*>(blobs) + (size_t)p * stride +
                                                   hs[(size_t)p].off_values);
            a.bounds = bounds + bo;
            a.G = v.g.G;
            a.gk_off = (int32_t)ko;   // < 2^31: the batch's keys fit the 3 GB scratch budget
            a.gb_off = (int32_t)bbo;
            // the run bounds come from the key query unless SKML_FORM_RUN_BOUNDS = 1 asks for the
            // separate k_agg_bounds pass (A/B)
#ifdef SKML_AB
            const bool own_pass = form(SKML_FORM_RUN_BOUNDS) == 1;
#else
            constexpr bool own_pass = false;
#endif
            const DecodeValues dv{a.nq, const_cast<void*>(a.gb), a.bw, err,
                                  own_pass ? RunBoundsOut{nullptr, 0, 0, 0}
                                           : RunBoundsOut{const_cast<int32_t*>(a.bounds), ntiles, dim, tile_bits}};
            auto join = [&](int e) {  // an error after the fork: the caller's stream still waits for the side
                if (lanes[1]) {
                    (void)hipEventRecord(ev_join, side_st);
                    (void)hipStreamWaitEvent(st, ev_join, 0);
                }
                return e;
            };
            if (int e = decode_groups(lc, &v, gk + ko, nullptr, true, &dv)) return join(e);
            if (v.nnz > lim) {  // live <= nnz: only then can toAuto pick the dense form
                if (launch_count_live(ls, a.gb, a.bw, v.nnz, a.qv, llive) != hipSuccess)
                    return join(fail(SKML_E_HIP, "count_live launch failed"));
                uint64_t nlive = 0;
                if (int e = sync_to_host(lc, &nlive, llive, sizeof(nlive))) return join(e);
                a.dense_form = (int64_t)nlive > lim ? 1 : 0;
            }
#ifdef SKML_AB
            if (own_pass && launch_agg_bounds(ls, a.gk, v.nnz, v.g_dev, ntiles, dim, const_cast<int32_t*>(a.bounds), err,
                                              tile_bits) != hipSuccess)
                return join(fail(SKML_E_HIP, "agg_bounds launch failed"));
#endif
            pays.push_back(a);
            ko += key_words(p);
            bbo += bin_bytes(p);
            bo += (int64_t)v.g.G * (ntiles + 1);
        }
        if (lanes[1]) {
            HIP_TRY(hipEventRecord(ev_join, side_st));
            HIP_TRY(hipStreamWaitEvent(st, ev_join, 0));
        }
        const bool last = end == todo.size();
        HIP_TRY(hipMemcpyAsync(d_pays, pays.data(), sizeof(AggPayload) * pays.size(), hipMemcpyHostToDevice, st));
        // the wave-tile form takes 8 payloads per launch (a lane per (payload, group)); later
        // launches continue the sum in payload order
        const size_t chunk = vt ? (size_t)kAggVPayloads : pays.size();
        for (size_t c0 = 0; c0 < pays.size(); c0 += chunk) {
            const size_t nc = std::min(chunk, pays.size() - c0);
            bool any_dense = false;
            for (size_t q = c0; q < c0 + nc; q++) any_dense |= pays[q].dense_form != 0;
            const int from_out = first && c0 == 0 ? 0 : 1;
            const bool final_launch = last && c0 + nc == pays.size();
            t_sum_launches++;
            if constexpr (std::is_same<O, double>::value) {
                HIP_TRY(launch_agg_tiles(st, d_pays + c0, (int)nc, ntiles, dim, out, from_out,
                                         final_launch ? scale : 1.0, err, vt, gk, gbn, any_dense));
            } else if (final_launch) {
                HIP_TRY(launch_agg_last(st, d_pays + c0, (int)nc, ntiles, dim, out, accd, from_out, scale, err, vt, gk,
                                        gbn, any_dense));
            } else {
                if (!accd && !(accd = scratch<double>(c, kSlotAggAcc, (size_t)dim)))
                    return fail(SKML_E_OOM, "decode_sum accumulator (%lld doubles)", (long long)dim);
                HIP_TRY(launch_agg_tiles(st, d_pays + c0, (int)nc, ntiles, dim, accd, from_out, 1.0, err, vt, gk, gbn,
                                         any_dense));
            }
        }
        HIP_TRY(hipStreamSynchronize(st));  // `pays` (host) and the scratch are reused by the next batch
        first = false;
        at = end;
    }
    unsigned bad = 0;
    if (int e = sync_to_host(c, &bad, err, sizeof(bad))) return e;
    if (bad & 1u)
        return fail(SKML_E_ARG, "a payload holds a key outside [0, %lld), a non-ascending run or a bin outside its "
                                "values (SparseDoubleGradient requires ascending indices in range)", (long long)dim);
    if (bad & 2u)
        return fail(SKML_E_ARG, "requirement failed: Indices are not strictly increasing (a key repeated across a "
                                "payload's groups; SparseDoubleGradient.scala:12)");
    return SKML_OK;
}

}  // namespace

extern "C" {

int skml_sparse_decode_sum_f64(skml_ctx* c, const void* blobs, int32_t P, size_t stride, int64_t dim, double scale,
                               double* out) {
    return decode_sum_any<double>(c, blobs, P, stride, dim, scale, out);
}

int skml_sparse_decode_sum_f32(skml_ctx* c, const void* blobs, int32_t P, size_t stride, int64_t dim, double scale,
                               float* out) {
    return decode_sum_any<float>(c, blobs, P, stride, dim, scale, out);
}

int skml_sparse_decode_sum_bf16(skml_ctx* c, const void* blobs, int32_t P, size_t stride, int64_t dim, double scale,
                                uint16_t* out) {
    return decode_sum_any<bf16_t>(c, blobs, P, stride, dim, scale, reinterpret_cast<bf16_t*>(out));
}

int skml_sparse_decode_sum_f16(skml_ctx* c, const void* blobs, int32_t P, size_t stride, int64_t dim, double scale,
                               uint16_t* out) {
    return decode_sum_any<f16_t>(c, blobs, P, stride, dim, scale, reinterpret_cast<f16_t*>(out));
}

}  // extern "C"
