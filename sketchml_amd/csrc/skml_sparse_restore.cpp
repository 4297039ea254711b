// skml_sparse_restore.cpp -- the restore side of the sparse C ABI (include/skml.h, "Sparse path"):
// GroupedMinMaxSketch.restore (frequency/GroupedMinMaxSketch.java:123-146), Sort.merge of the
// groups' runs and SparseVectorCompressor.decompressSparse (sample/SparseVectorCompressor.java:
// 118-126).  All element work runs in skml_sparse*.hip; the host plans the launches.
#include <algorithm>
#include <vector>

#include "skml_sparse_host.hpp"

using namespace skml;

namespace skml {

int decode_groups(skml_ctx* c, const skml_sparse* s, int32_t* gk, int32_t* gb, bool query, const DecodeValues* dv,
                  const RunBoundsOut* rbo) {
    hipStream_t st = c->stream;
    const SpGroups& G = s->g;
    const int64_t n = s->nnz;
    bool any_unary = false;
    for (int g = 0; g < G.G; g++) any_unary |= G.kind[g] && G.gstart[g + 1] > G.gstart[g];
    int64_t* end_pos = nullptr;
    if (any_unary) {
        end_pos = scratch<int64_t>(c, kSlotEndPos, (size_t)n);
        const int64_t wt = sp_tiles(s->n_flag_words, kSpTile);
        uint64_t* ts = scratch<uint64_t>(c, kSlotTiles, (size_t)(wt + 1));
        if (!end_pos || !ts) return fail(SKML_E_OOM, "decode scratch");
        HIP_TRY(launch_unary_count(st, s->flag_words, s->n_flag_words, s->g_dev, ts));
        if (int e = scan_tiles(c, ts, wt, 1, nullptr)) return e;
        HIP_TRY(launch_unary_select(st, s->flag_words, s->n_flag_words, s->g_dev, ts, end_pos));
    }
    const int64_t tiles = sp_tiles(n, kSpTile);
    uint64_t* ts = scratch<uint64_t>(c, kSlotTiles, (size_t)(tiles + 1) * 2);
    uint64_t* gpre = scratch<uint64_t>(c, kSlotSmall, kMaxGroups + 8);
    if (!ts || !gpre) return fail(SKML_E_OOM, "decode scratch");
    uint64_t* ts2 = ts + (tiles + 1);
    uint8_t* dlen = scratch<uint8_t>(c, kSlotNeed, (size_t)n);
    uint32_t* delta = scratch<uint32_t>(c, kSlotDelta, (size_t)n);
    if (!dlen || !delta) return fail(SKML_E_OOM, "decode scratch");
    // the query gathers from a byte (binNum <= 256) or 16-bit image of the tables, built by extra
    // blocks of the lengths' launch
    const int32_t* tab = query ? s->tables : nullptr;
    int width = 32;
    void* tnar = nullptr;
    if (query && s->tnar && s->ncells > 0) {  // the payload's exact image (encoder or blob): gathered as is
        tab = nullptr;
        width = s->tnar_width;
        tnar = s->tnar;
    } else if (tab && s->ncells > 0 && (reinterpret_cast<uintptr_t>(tab) & 15) == 0) {
        width = G.bin_num <= 256 ? 8 : 16;  // any width gives the same bins (the sentinel reads back)
        tnar = ctx_scratch(c, kSlotNarrowTab, (size_t)s->ncells * (size_t)(width / 8));
        if (!tnar) return fail(SKML_E_OOM, "decode scratch (table image)");
    }
    // three passes (lengths, their tile scan, deltas); SKML_FORM_DEC_LOOKBACK = 1: one pass with
    // decoupled look-backs for the bit offsets and the deltas' prefixes, 2: the same pass with the
    // deltas' tile scan after it (A/B forms, measured slower: the look-back chain across 13 K tiles
    // ran 230 us against 107 us for the three passes, profiles/ab/r05_dec_lookback.txt)
#ifdef SKML_AB
    const int lb = form(SKML_FORM_DEC_LOOKBACK);
    const int split = lb == 1 ? 0 : lb == 2 ? 2 : 1;
#else
    constexpr int split = 1;
#endif
    if (split == 1) {
        HIP_TRY(launch_dec_lens(st, s->flag_words, s->n_flag_words, end_pos, n, s->g_dev, dlen, ts,
                                NarrowJob{tab, s->ncells, tab ? tnar : nullptr, width}));
        if (int e = scan_tiles(c, ts, tiles, 1, nullptr)) return e;
        HIP_TRY(launch_dec_deltas(st, s->delta_words, s->n_delta_words, dlen, n, s->g_dev, ts, delta, ts2));
    } else {
#ifdef SKML_AB
        uint64_t* status = scratch<uint64_t>(c, kSlotLookback, 2 * (size_t)tiles + 8);
        if (!status) return fail(SKML_E_OOM, "decode scratch (look-back)");
        HIP_TRY(launch_dec_lens_deltas(st, s->flag_words, s->n_flag_words, end_pos, n, s->g_dev, s->delta_words,
                                       s->n_delta_words, delta, ts2, status, NarrowJob{tab, s->ncells, tab ? tnar : nullptr, width},
                                       split == 0));
#endif
    }
    if (split != 0)
        if (int e = scan_tiles(c, ts2, tiles, 1, nullptr)) return e;
    HIP_TRY(launch_group_prefix(st, delta, n, s->g_dev, G.G, ts2, gpre));
    HIP_TRY(launch_dec_keys(st, delta, n, s->g_dev, G, ts2, gpre, tab, tnar, width, gk, gb, dv ? dv->nq : 0,
                            dv ? dv->gb : nullptr, dv ? dv->bw : 0, dv ? dv->err : nullptr,
                            dv ? dv->rb : rbo ? *rbo : RunBoundsOut{nullptr, 0, 0, 0}));
    return SKML_OK;
}

int merge_groups(skml_ctx* c, const skml_sparse* s, int32_t* gk, int32_t* gb, int32_t* keys_out,
                 int32_t* bins_out) {
    hipStream_t st = c->stream;
    const int64_t n = s->nnz;
    const SpGroups& G = s->g;
    int32_t* k1 = scratch<int32_t>(c, kSlotK1, (size_t)n);
    int32_t* b1 = scratch<int32_t>(c, kSlotB1, (size_t)n);
    if (!k1 || !b1) return fail(SKML_E_OOM, "merge scratch");
    // every round's run offsets (the rounds halve the run count) go to the kernels by value
    std::vector<int64_t> rs(G.gstart, G.gstart + G.G + 1);
    int64_t* split = rs.size() > 2 ? scratch<int64_t>(c, kSlotEndPos, (size_t)sp_tiles(n, kSpTile) + 2) : nullptr;
    if (rs.size() > 2 && !split) return fail(SKML_E_OOM, "merge split points");
    int32_t *kin = gk, *bin = gb, *kout = k1, *bout = b1;
    // the last round writes straight into the outputs (bins too unless bins_out is a scratch buffer)
    const bool bins_direct = bins_out && bins_out != gb && bins_out != b1;
    bool keys_done = false, bins_done = false;
    while (rs.size() > 2) {
        const bool last = rs.size() <= 3;
        int32_t* ko = last ? keys_out : kout;
        int32_t* bo = last && bins_direct ? bins_out : bout;
        HIP_TRY(launch_merge_round(st, kin, bin, ko, bo, rs.data(), (int)rs.size() - 1, n, split));
        std::vector<int64_t> nx;
        for (size_t i = 0; i < rs.size(); i += 2) nx.push_back(rs[i]);
        if (nx.back() != rs.back()) nx.push_back(rs.back());
        rs.swap(nx);
        keys_done = last;
        bins_done = last && bins_direct;
        kin = ko;
        bin = bo;
        kout = kin == k1 ? gk : k1;
        bout = bin == b1 ? gb : b1;
    }
    if (!keys_done) HIP_TRY(hipMemcpyAsync(keys_out, kin, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    if (!bins_done && bins_out && bins_out != bin)
        HIP_TRY(hipMemcpyAsync(bins_out, bin, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    return SKML_OK;
}

int rs_merge_prepare(skml_ctx* c, const skml_sparse* s, RsMerge* m) {
    *m = RsMerge{};
    if (s->g.G < 2 || form(SKML_FORM_RS_ROUNDS) == 1) return SKML_OK;
    const size_t o_b = align_up(sizeof(RsInfo), 256);
    char* blk = static_cast<char*>(
        ctx_scratch(c, kSlotRsMerge, o_b + sizeof(int32_t) * (size_t)s->g.G * (size_t)(kRsRanges + 1)));
    if (!blk) return fail(SKML_E_OOM, "merge scratch");
    HIP_TRY(hipMemsetAsync(blk, 0, o_b, c->stream));  // whole 256-byte units: one fill
    m->info = reinterpret_cast<RsInfo*>(blk);
    m->bounds = reinterpret_cast<int32_t*>(blk + o_b);
    return SKML_OK;
}

int rs_merge_start(skml_ctx* c, const skml_sparse* s, const RsMerge& m, const int32_t* gk, const int32_t* gb,
                   int32_t* keys_out, void* out, int vkind, const double* qv, int nq, volatile unsigned** pending) {
    *pending = nullptr;
    if (!m.info) return SKML_OK;
    hipStream_t st = c->stream;
    unsigned* pin = static_cast<unsigned*>(ctx_pinned(c, 64));
    if (!pin) return fail(SKML_E_OOM, "merge scratch");
    HIP_TRY(launch_rs_merge(st, gk, gb, s->nnz, s->g_dev, m.bounds, m.info, keys_out, out, vkind, qv, nq, m.by_query));
    HIP_TRY(hipMemcpyAsync(pin, &m.info->irregular, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    *pending = pin;
    return SKML_OK;
}

}  // namespace skml

namespace {
// restore + Sort.merge + quantValues[bin] (SparseVectorCompressor.decompressSparse,
// SparseVectorCompressor.java:118-126) as fp32 or as the reference's doubles
template <typename T>
int decode_values(skml_ctx* c, const skml_sparse* s, int32_t* keys_dev, T* vals_dev) {
    if (!c || !s) return fail(SKML_E_ARG, "bad decode arguments");
    const int64_t n = s->nnz;
    if (n == 0) return SKML_OK;
    if (!keys_dev || !vals_dev) return fail(SKML_E_ARG, "keys/vals are NULL");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (s->qvalues.empty()) return fail(SKML_E_STATE, "quantValues are not set (deserialised without them)");
    int32_t* gk = scratch<int32_t>(c, kSlotGKeys, (size_t)n);
    int32_t* gb = scratch<int32_t>(c, kSlotGBins, (size_t)n);
    int32_t* b1 = scratch<int32_t>(c, kSlotB1, (size_t)n);
    if (!gk || !gb || !b1) return fail(SKML_E_OOM, "decode scratch");
    // the value table's upload and the merge's RsInfo fill go first: the GPU runs them while the
    // decode's kernels are still being queued
    const int nq = (int)s->qvalues.size();
    double* qv = s->qv_dev;  // the payload's device copy (encode / import), or the host table uploaded
    if (!qv || !s->qv_dev_ok) {
        if (!qv) qv = reinterpret_cast<double*>(ctx_scratch(c, kSlotCells, sizeof(double) * s->qvalues.size()));
        if (!qv) return fail(SKML_E_OOM, "value table");
        HIP_TRY(hipMemcpyAsync(qv, s->qvalues.data(), sizeof(double) * s->qvalues.size(), hipMemcpyHostToDevice, st));
        if (qv == s->qv_dev) const_cast<skml_sparse*>(s)->qv_dev_ok = true;  // ordered before later restores
    }
    RsMerge rm;
    if (int e = rs_merge_prepare(c, s, &rm)) return e;
    const RunBoundsOut rbo = rm.query_bounds();  // the merge's key-range bounds from the query
    if (int e = decode_groups(c, s, gk, gb, true, nullptr, &rbo)) return e;
    // pairwise merge rounds, then quantValues[bin]; a bin outside the nq values (Java: index out
    // of bounds) fails the decode (the one-pass merge sends such input here too)
    auto rounds = [&]() -> int {
        unsigned* err = scratch<unsigned>(c, kSlotStatus, 64);
        if (!err) return fail(SKML_E_OOM, "decode scratch");
        HIP_TRY(hipMemsetAsync(err, 0, sizeof(unsigned), st));
        if (int e = merge_groups(c, s, gk, gb, keys_dev, b1)) return e;
        if constexpr (sizeof(T) == 8) HIP_TRY(launch_bin_values64(st, b1, n, qv, nq, vals_dev, err));
        else HIP_TRY(launch_bin_values(st, b1, n, qv, nq, vals_dev, err));
        unsigned bad = 0;
        if (int e = sync_to_host(c, &bad, err, sizeof(bad))) return e;
        return bad ? fail(SKML_E_ARG, "a restored bin lies outside the %d quantValues", nq) : SKML_OK;
    };
    volatile unsigned* pending = nullptr;
    if (int e = rs_merge_start(c, s, rm, gk, gb, keys_dev, vals_dev, sizeof(T) == 8 ? 2 : 1, qv, nq, &pending))
        return e;
    if (!pending) {
        t_merge_path = s->g.G < 2 ? 0 : 2;
        return rounds();
    }
    HIP_TRY(hipStreamSynchronize(st));
    t_merge_path = 1;
    if (*pending) {  // not regular, or a bin outside quantValues: the rounds decide
        t_merge_path = 3;
        return rounds();
    }
    return SKML_OK;
}
}  // namespace

extern "C" {

int skml_sparse_decode_f32(skml_ctx* c, const skml_sparse* s, int32_t* keys_dev, float* vals_dev) {
    return decode_values<float>(c, s, keys_dev, vals_dev);
}

int skml_sparse_decode_f64(skml_ctx* c, const skml_sparse* s, int32_t* keys_dev, double* vals_dev) {
    return decode_values<double>(c, s, keys_dev, vals_dev);
}

// GroupedMinMaxSketch.restore (GroupedMinMaxSketch.java:123-146) + Sort.merge: keys and int32 bins.
int skml_sparse_restore_bins(skml_ctx* c, const skml_sparse* s, int32_t* keys_dev, int32_t* bins_dev) {
    if (!c || !s) return fail(SKML_E_ARG, "bad restore arguments");
    const int64_t n = s->nnz;
    if (n == 0) return SKML_OK;
    if (!keys_dev || !bins_dev) return fail(SKML_E_ARG, "keys/bins are NULL");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int32_t* gk = scratch<int32_t>(c, kSlotGKeys, (size_t)n);
    int32_t* gb = scratch<int32_t>(c, kSlotGBins, (size_t)n);
    if (!gk || !gb) return fail(SKML_E_OOM, "restore scratch");
    RsMerge rm;
    if (int e = rs_merge_prepare(c, s, &rm)) return e;
    const RunBoundsOut rbo = rm.query_bounds();  // the merge's key-range bounds from the query
    if (int e = decode_groups(c, s, gk, gb, true, nullptr, &rbo)) return e;
    volatile unsigned* pending = nullptr;
    if (int e = rs_merge_start(c, s, rm, gk, gb, keys_dev, bins_dev, 0, nullptr, 0, &pending)) return e;
    if (!pending)
        if (int e = merge_groups(c, s, gk, gb, keys_dev, bins_dev)) return e;
    HIP_TRY(hipStreamSynchronize(st));
    t_merge_path = s->g.G < 2 ? 0 : pending ? 1 : 2;
    if (pending && *pending) {  // not regular: the merge rounds decide
        t_merge_path = 3;
        if (int e = merge_groups(c, s, gk, gb, keys_dev, bins_dev)) return e;
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SKML_OK;
}

}  // extern "C"
