// skml_sparse_encode.cpp -- the encode side of the sparse C ABI (include/skml.h, "Sparse path"):
// SparseVectorCompressor.compressSparse (sample/SparseVectorCompressor.java:52-67) over
// GroupedMinMaxSketch.insert (frequency/GroupedMinMaxSketch.java:51-121), the toSparse compaction
// in front of it, and the standalone DeltaAdaptiveEncoder (binary/DeltaAdaptiveEncoder.java).  All
// element work runs in skml_sparse*.hip; the host plans launches, owns the per-group table and the
// tiny decisions the reference makes on whole-group statistics (colNum, hash choice, interval choice).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "skml_sparse_host.hpp"

using namespace skml;

namespace {

// Spin on the context's coherent host word until a kernel of this stream publishes a count >= 0
// there.  The stream is checked every few thousand polls, so a failed launch cannot hang the caller.
int wait_host_count(skml_ctx* c, const int64_t* word, int64_t* out) {
    const volatile int64_t* w = word;
    hipStream_t st = c->stream;
    for (uint64_t k = 1;; k++) {
        const int64_t v = *w;
        if (v >= 0) {
            *out = v;
            return SKML_OK;
        }
        if ((k & 4095) == 0) {
            const hipError_t e = hipStreamQuery(st);
            if (e == hipSuccess) {  // the stream has drained: the publishing store is visible now
                const int64_t v2 = *w;
                if (v2 < 0) return fail(SKML_E_HIP, "the compaction did not publish its count");
                *out = v2;
                return SKML_OK;
            }
            if (e != hipErrorNotReady) return fail(SKML_E_HIP, "stream failed: %s", hipGetErrorString(e));
        }
        __builtin_ia32_pause();
    }
}

// Worst-case stream words of n keys: 17 flag bits (unary, 16 intervals) and 32 delta bits each,
// the trailing word, and the edge words' slack.
inline int64_t flag_words_max(int64_t n) { return (17 * n + 63) / 64 + 3; }
inline int64_t delta_words_max(int64_t n) { return (32 * n + 63) / 64 + 3; }

// DeltaAdaptiveEncoder.encode (binary/DeltaAdaptiveEncoder.java:54-109) of every group of g_dev
// over the grouped keys gk (n of them), all on the stream: interval choice from the bitsNeeded
// histogram, bit lengths, their scan, the edge words, the writer, the group bases.
int encode_delta_device(skml_ctx* c, hipStream_t st, SpGroups* g_dev, const int32_t* gk, const uint8_t* need,
                        int64_t n, const uint32_t* hist, const uint32_t* err, uint64_t* fw, uint64_t* dw) {
    const int64_t tiles = sp_tiles(n, kSpTile);
    uint64_t* ts = scratch<uint64_t>(c, kSlotTiles, (size_t)(tiles + 1) * 2);
    if (!ts) return fail(SKML_E_OOM, "tile sums");
    HIP_TRY(launch_sp_plan_delta(st, g_dev, hist, err));
    HIP_TRY(launch_delta_lens(st, need, n, g_dev, ts));
    HIP_TRY(launch_scan_cols_small(st, ts, tiles, 2));
    HIP_TRY(launch_sp_zero_edges(st, ts, tiles, g_dev, fw, dw));
    HIP_TRY(launch_delta_write(st, gk, need, n, g_dev, ts, fw, dw));
    HIP_TRY(launch_sp_finalize(st, g_dev, ts + tiles * 2));
    return SKML_OK;
}

int check_params(const skml_params* p) {
    if (!p) return fail(SKML_E_ARG, "params is NULL");
    if (p->bin_num < 2 || p->bin_num > SKML_MAX_BINS)
        return fail(SKML_E_ARG, "bin_num %d outside [2, %d]", p->bin_num, SKML_MAX_BINS);
    if (p->group_num < 2 || p->group_num > kMaxGroups)
        return fail(SKML_E_ARG, "group_num %d outside [2, %d]", p->group_num, kMaxGroups);
    if (p->row_num < 1 || p->row_num > kMaxRows)
        return fail(SKML_E_ARG, "Currently only %d hash functions are available", kMaxRows);
    if (!(p->col_ratio > 0.0)) return fail(SKML_E_ARG, "col_ratio must be positive");
    if (p->quant_type != SKML_QUANTILE && p->quant_type != SKML_UNIFORM)
        return fail(SKML_E_ARG, "Unrecognizable quantization type: %d", p->quant_type);
    if (p->parallelism < 0 || p->parallelism > 65536)
        return fail(SKML_E_ARG, "Invalid parallelism: %d", p->parallelism);
    return SKML_OK;
}

// SparseVectorCompressor.compressSparse (sample/SparseVectorCompressor.java:52-67) over
// GroupedMinMaxSketch.insert (frequency/GroupedMinMaxSketch.java:51-121).  Everything is queued
// on the stream without a host round trip -- the per-group decisions are made on the device
// (k_sp_plan_*) -- and the host reads the quantizer header, splits and group table back once.
// vals: nnz floats, or nnz doubles when f64 (the reference's own double[] values: the quantizer
// sketches and bins the doubles themselves, QuantileQuantizer.quantize(double[])).
// A failing encode leaves through `own`, which synchronises the stream (and the DeltaAdaptive
// chain's, once forked) before the block returns to the pool: nothing may still use it.
int encode_kv(skml_ctx* c, const int32_t* keys, const void* vals, bool f64, int64_t nnz, const skml_params* p,
              skml_sparse** out) {
    hipStream_t st = c->stream;
    skml_sparse* s = new skml_sparse();
    PayloadOwner own(s, st);
    s->device = c->device;
    s->nnz = nnz;
    s->params = *p;
    const int G = p->group_num, rows = p->row_num;
    // ---- the payload's device block, sized for the worst case (no count has to come back first) ----
    const double cols_all = std::ceil((double)nnz * p->col_ratio);
    if (cols_all * rows > 4.0e12) return fail(SKML_E_OOM, "MinMaxSketch tables of colRatio %g", p->col_ratio);
    const int64_t cells_max = nnz > 0 ? (int64_t)rows * ((int64_t)cols_all + 2 * G + 2) : 0;
    const int64_t fwn = flag_words_max(nnz), dwn = delta_words_max(nnz);
    s->qbytes = skml_dense_payload_bytes(nnz, p->bin_num);
    const size_t o_g = align_up(s->qbytes, 256);
    const size_t o_tab = o_g + align_up(sizeof(SpGroups), 256);
    // the tables' exact narrow image: 16 bits a cell reserved (the effective bin count, which picks
    // 8 or 16, is known on the device only)
    const bool want_tn = tnar_width_for(p->bin_num) != 0;
    const size_t o_tn = o_tab + align_up(sizeof(int32_t) * (size_t)std::max<int64_t>(cells_max, 1), 256);
    const size_t o_fw = o_tn + (want_tn ? align_up(sizeof(uint16_t) * (size_t)std::max<int64_t>(cells_max, 1), 256) : 0);
    const size_t o_dw = o_fw + align_up(sizeof(uint64_t) * (size_t)fwn, 256);
    const size_t o_qv = o_dw + align_up(sizeof(uint64_t) * (size_t)dwn, 256);
    const size_t total = o_qv + sizeof(double) * (size_t)p->bin_num;
    char* blk = static_cast<char*>(block_get(s->device, total, &s->block_cap));
    if (!blk) return fail(SKML_E_OOM, "sparse payload of %zu bytes", total);
    s->block = blk;
    s->qpayload = blk;
    s->qv_dev = reinterpret_cast<double*>(blk + o_qv);
    s->g_dev = reinterpret_cast<SpGroups*>(blk + o_g);
    s->tables = reinterpret_cast<int32_t*>(blk + o_tab);
    s->tnar = want_tn ? blk + o_tn : nullptr;
    s->flag_words = reinterpret_cast<uint64_t*>(blk + o_fw);
    s->delta_words = reinterpret_cast<uint64_t*>(blk + o_dw);
    // ---- 1. the values' quantizer (Quantizer.newQuantizer(quantType), SparseVectorCompressor.java:60-62) ----
    skml_params qp = *p;
    int qe;
    if (f64) {
        const double* v = static_cast<const double*>(vals);
        qe = p->quant_type == SKML_UNIFORM ? skml_dense_encode_uniform_f64(c, v, nnz, &qp, s->qpayload, s->qbytes)
             : p->parallelism > 1 ? skml_dense_encode_parallel_f64(c, v, nnz, p->parallelism, &qp, s->qpayload, s->qbytes)
                                  : skml_dense_encode_f64(c, v, nnz, &qp, s->qpayload, s->qbytes);
    } else {
        const float* v = static_cast<const float*>(vals);
        qe = p->quant_type == SKML_UNIFORM ? skml_dense_encode_uniform_f32(c, v, nnz, &qp, s->qpayload, s->qbytes)
             : p->parallelism > 1 ? skml_dense_encode_parallel_f32(c, v, nnz, p->parallelism, &qp, s->qpayload, s->qbytes)
                                  : skml_dense_encode_f32(c, v, nnz, &qp, s->qpayload, s->qbytes);
    }
    if (qe) return qe;
    // ---- 2. group edges (device), partition counts, per-group MinMaxSketch shapes ----
    SpInit init{};
    init.G = G;
    init.rows = rows;
    // The staged scatter needs the pairs' hashed cells (int32, under 2^31 cells) and the per-(tile,
    // bucket) reservations (under 2^31 pairs).  Both scratch buffers are taken here, before
    // k_sp_plan_edges chooses narrow pairs, so narrow_ok follows what was actually allocated: when
    // either allocation fails the encode takes the rehashing, key-carrying scatter instead of failing.
    const int nbuckets = (int)((cells_max + kMmCellsPerBucket - 1) / kMmCellsPerBucket);
    const bool reserve = (uint64_t)rows * (uint64_t)nnz < (1ull << 31);
    const int64_t mm_tiles = sp_tiles(nnz, mm_chunk(nnz));  // the tiles k_group_prep / the scatter use
    const bool staging = !g_fail_cellbuf.load();
    uint32_t* tile_off =
        reserve && staging ? scratch<uint32_t>(c, kSlotTileOff, (size_t)mm_tiles * (size_t)nbuckets) : nullptr;
    int32_t* cellbuf =
        cells_max < INT32_MAX && staging ? scratch<int32_t>(c, kSlotCellIdx, (size_t)rows * (size_t)nnz) : nullptr;
    init.narrow_ok = mm_scatter_staged(cellbuf != nullptr, tile_off != nullptr, nbuckets) ? 1 : 0;
    init.col_ratio = p->col_ratio;
    for (int g = 0; g < G; g++) pick_hashes(p->hash_seed + g, rows, init.hash_ids[g]);
    SP_TRY(launch_sp_plan_edges(st, s->qpayload, init, s->g_dev));
    const int64_t tiles = sp_tiles(nnz, kSpTile);
    uint64_t* tc = scratch<uint64_t>(c, kSlotTiles, (size_t)(tiles + 1) * G);
    if (!tc) return fail(SKML_E_OOM, "tile counts");
    // partition counts; the grid also zeroes the histogram, error flag and bucket counters below
    uint64_t* bucket = scratch<uint64_t>(c, kSlotCells, (size_t)2 * nbuckets + 2);  // counts->bases, cursors
    uint32_t* small = scratch<uint32_t>(c, kSlotSmall, (size_t)kMaxGroups * kDeltaHist + 64);
    if (!bucket || !small) return fail(SKML_E_OOM, "sparse scratch");
    SP_TRY(launch_part_count(st, s->qpayload, nnz, s->g_dev, tc, small, (int64_t)kMaxGroups * kDeltaHist + 64, bucket,
                             (int64_t)2 * nbuckets + 2));
    SP_TRY(launch_scan_cols_major(st, tc, tiles, G));
    SP_TRY(launch_sp_plan_groups(st, s->g_dev, tc + tiles, tiles + 1));
    // ---- 3. partition, deltas / histogram / order check, bucketed MinMax insert ----
    int32_t* gk = scratch<int32_t>(c, kSlotGKeys, (size_t)nnz);
    uint16_t* gb = scratch<uint16_t>(c, kSlotGBins, (size_t)nnz);  // grouped bins (< 65536)
    uint8_t* need = scratch<uint8_t>(c, kSlotNeed, (size_t)nnz);
    // reserved ranges are padded to 16 wide (u64) or 32 narrow (u32) pairs
    const size_t npairs = (size_t)rows * (size_t)nnz + (tile_off ? (size_t)15 * mm_tiles * nbuckets : 0);
    const size_t npairs32 = (size_t)rows * (size_t)nnz + (tile_off ? (size_t)31 * mm_tiles * nbuckets : 0);
    uint64_t* pairs = scratch<uint64_t>(c, kSlotDelta, std::max(npairs, (npairs32 + 1) / 2));
    if (!gk || !gb || !need || !pairs) return fail(SKML_E_OOM, "sparse scratch");
    uint64_t* cursor = bucket + nbuckets + 1;
    uint32_t* hist = small;
    uint32_t* err = small + kMaxGroups * kDeltaHist;
    SP_TRY(launch_part_scatter(st, keys, s->qpayload, nnz, s->g_dev, tc, gk, gb));
    SP_TRY(launch_group_prep(st, gk, nnz, s->g_dev, need, hist, err, bucket, nbuckets, cellbuf, tile_off));
    // ---- 4. DeltaAdaptive key streams on the side stream, beside the MinMax scatter and minima:
    // the VALU-bound stream writer runs while the scatter waits on memory.  The two chains touch
    // disjoint fields of the group table and disjoint buffers; the main stream joins before the
    // read-back.  (Forking before the count pass instead, with the deltas and histogram computed
    // on the side, overlapped the two VALU-bound passes and was slower.) ----
    hipStream_t side = nullptr;  // the DeltaAdaptive chain's stream, once forked
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t ds = st;
    if (nnz > 0 && ctx_side_fork(c, &side, &ev_fork, &ev_join) == SKML_OK) {
        own.side = side;
        SP_TRY(hipEventRecord(ev_fork, st));
        SP_TRY(hipStreamWaitEvent(side, ev_fork, 0));
        ds = side;
    } else {
        side = nullptr;
    }
    if (int e = encode_delta_device(c, ds, s->g_dev, gk, need, nnz, hist, err, s->flag_words, s->delta_words))
        return e;
    // quantValues on the device (only restores read them): on the side chain, off the critical path
    SP_TRY(launch_sp_qvalues(ds, s->qpayload, s->qv_dev));
    if (side) SP_TRY(hipEventRecord(ev_join, side));
    SP_TRY(launch_scan_cols(st, bucket, nbuckets, 1));
    SP_TRY(launch_mm_scatter(st, gk, gb, nnz, s->g_dev, bucket, cursor, nbuckets, pairs, cellbuf, tile_off));
    SP_TRY(launch_mm_bucket(st, pairs, bucket, nbuckets, s->g_dev, s->tables, s->tnar));
    if (side) SP_TRY(hipStreamWaitEvent(st, ev_join, 0));
    // ---- 5. the one read-back: quantizer header and splits, group table ----
    const size_t qh = kHeaderBytes + sizeof(double) * (size_t)(p->bin_num - 1);
    const size_t o_pg = align_up(qh, 256);
    uint8_t* pin = static_cast<uint8_t*>(ctx_pinned(c, o_pg + sizeof(SpGroups)));
    if (!pin) return fail(SKML_E_OOM, "pinned staging");
    SP_TRY(hipMemcpyAsync(pin, s->qpayload, qh, hipMemcpyDeviceToHost, st));
    SP_TRY(hipMemcpyAsync(pin + o_pg, s->g_dev, sizeof(SpGroups), hipMemcpyDeviceToHost, st));
    SP_TRY(hipStreamSynchronize(st));
    std::memcpy(&s->hdr, pin, sizeof(skml_dense_header));
    std::memcpy(&s->g, pin + o_pg, sizeof(SpGroups));
    if (s->hdr.status == SKML_E_NAN || (s->g.status & kSpNan)) return fail(SKML_E_NAN, "Encounter NaN value");
    if (s->g.status & kSpEdges) {
        int32_t e_host[kMaxGroups];
        const int e = report(group_edges(s->hdr.zero_idx, s->hdr.bin_num, G, e_host));
        return e ? e : fail(SKML_E_HIP, "group plan disagrees with calGroupEdges");
    }
    if (s->g.status & kSpOrder)
        return fail(SKML_E_ORDER, "Log for a non-positive key delta (keys must ascend strictly)");
    {  // Quantizer.getValues (base/Quantizer.java:39-47)
        const int B = s->hdr.bin_num, ns = B - 1;
        const double* sp = reinterpret_cast<const double*>(pin + kHeaderBytes);
        s->splits.assign(sp, sp + std::max(ns, 0));
        s->qvalues.resize((size_t)B);
        for (int b = 0; b < B; b++) {
            double v;
            if (b == 0) v = 0.5 * (s->hdr.min + s->splits[0]);
            else if (b == ns) v = 0.5 * (s->splits[ns - 1] + s->hdr.max);
            else v = 0.5 * (s->splits[b - 1] + s->splits[b]);
            s->qvalues[(size_t)b] = v;
        }
    }
    s->qv_dev_ok = true;
    s->ncells = s->g.ncells;
    s->tnar_width = s->tnar ? tnar_width_for(s->g.bin_num) : 0;
    if (!s->tnar_width) s->tnar = nullptr;
    s->flag_bits = s->g.fb[G];
    s->delta_bits = s->g.db[G];
    s->n_flag_words = (s->flag_bits + 63) / 64 + 1;
    s->n_delta_words = (s->delta_bits + 63) / 64 + 1;
    own.release(out);
    return SKML_OK;
}

// poll: the count goes to the context's host word and the call returns as soon as it is there,
// with the kernel's last stores possibly still in flight -- only for callers whose next work
// runs on the same stream (skml_sparse_encode_*); the public compaction synchronises.
// T: the dense values' type; V: the compacted values' (T itself, or float for bf16 / fp16 storage).
template <typename T, typename V = T>
int compact_any(skml_ctx* c, const T* dense, int64_t dim, int32_t* keys, V* vals, int64_t* nnz_out,
                bool poll = false) {
    if (!c || !nnz_out || dim < 0 || (dim > 0 && (!dense || !keys || !vals)))
        return fail(SKML_E_ARG, "bad compaction arguments");
    if (dim > (int64_t)INT32_MAX) return fail(SKML_E_ARG, "dim %lld exceeds Java int keys", (long long)dim);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t tiles = sp_tiles(dim, sizeof(T) == 8 ? kCompactTile / 2 : kCompactTile);
    uint64_t* status = scratch<uint64_t>(c, kSlotStatus, (size_t)tiles + 8);
    if (!status) return fail(SKML_E_OOM, "compaction status");
    unsigned* ticket = reinterpret_cast<unsigned*>(status + tiles);
    int64_t* nnz_dev = reinterpret_cast<int64_t*>(status + tiles + 1);
    int64_t* hw = poll && tiles > 0 ? ctx_host_word(c) : nullptr;
    if (hw) *reinterpret_cast<volatile int64_t*>(hw) = -1;
    HIP_TRY(hipMemsetAsync(status, 0, sizeof(uint64_t) * ((size_t)tiles + 8), st));
    int64_t* dst = hw ? hw : nnz_dev;
    if constexpr (sizeof(T) == 8) HIP_TRY(launch_compact64(st, dense, dim, keys, vals, status, ticket, dst));
    else HIP_TRY(launch_compact(st, dense, dim, keys, vals, status, ticket, dst));
    if (hw) return wait_host_count(c, hw, nnz_out);
    return sync_to_host(c, nnz_out, nnz_dev, sizeof(int64_t));
}

// X: float, or bf16 / fp16 storage read as it is; the compacted values are fp32 either way
template <typename X>
int encode_dense_x(skml_ctx* c, const X* dense, int64_t dim, const skml_params* p, skml_sparse** out) {
    if (!c || !out || dim < 0) return fail(SKML_E_ARG, "bad sparse arguments");
    if (int e = check_params(p)) return e;
    HIP_TRY(hipSetDevice(c->device));
    const size_t cap = (size_t)std::max<int64_t>(dim, 1);
    int32_t* keys = scratch<int32_t>(c, kSlotCKeys, cap);
    float* vals = scratch<float>(c, kSlotCVals, cap);
    if (!keys || !vals) return fail(SKML_E_OOM, "compaction output");
    int64_t nnz = 0;
    if (int e = compact_any<X, float>(c, dense, dim, keys, vals, &nnz, true)) return e;
    return encode_kv(c, keys, vals, false, nnz, p, out);
}

}  // namespace

extern "C" {

int skml_sparse_compact_f32(skml_ctx* c, const float* dense, int64_t dim, int32_t* keys, float* vals,
                            int64_t* nnz_out) {
    return compact_any<float>(c, dense, dim, keys, vals, nnz_out);
}

int skml_sparse_compact_f64(skml_ctx* c, const double* dense, int64_t dim, int32_t* keys, double* vals,
                            int64_t* nnz_out) {
    return compact_any<double>(c, dense, dim, keys, vals, nnz_out);
}

int skml_sparse_compact_bf16(skml_ctx* c, const uint16_t* dense, int64_t dim, int32_t* keys, float* vals,
                             int64_t* nnz_out) {
    return compact_any<bf16_t, float>(c, reinterpret_cast<const bf16_t*>(dense), dim, keys, vals, nnz_out);
}

int skml_sparse_compact_f16(skml_ctx* c, const uint16_t* dense, int64_t dim, int32_t* keys, float* vals,
                            int64_t* nnz_out) {
    return compact_any<f16_t, float>(c, reinterpret_cast<const f16_t*>(dense), dim, keys, vals, nnz_out);
}

int skml_sparse_encode_kv_f32(skml_ctx* c, const int32_t* keys, const float* vals, int64_t nnz,
                              const skml_params* p, skml_sparse** out) {
    if (!c || !out || nnz < 0 || (nnz > 0 && (!keys || !vals))) return fail(SKML_E_ARG, "bad sparse arguments");
    if (nnz > (int64_t)INT32_MAX) return fail(SKML_E_ARG, "nnz exceeds Java int");
    if (int e = check_params(p)) return e;
    HIP_TRY(hipSetDevice(c->device));
    *out = nullptr;
    return encode_kv(c, keys, vals, false, nnz, p, out);
}

int skml_sparse_encode_kv_f64(skml_ctx* c, const int32_t* keys, const double* vals, int64_t nnz,
                              const skml_params* p, skml_sparse** out) {
    if (!c || !out || nnz < 0 || (nnz > 0 && (!keys || !vals))) return fail(SKML_E_ARG, "bad sparse arguments");
    if (nnz > (int64_t)INT32_MAX) return fail(SKML_E_ARG, "nnz exceeds Java int");
    if (int e = check_params(p)) return e;
    HIP_TRY(hipSetDevice(c->device));
    *out = nullptr;
    return encode_kv(c, keys, vals, true, nnz, p, out);
}

int skml_sparse_encode_f32(skml_ctx* c, const float* dense, int64_t dim, const skml_params* p,
                           skml_sparse** out) {
    return encode_dense_x<float>(c, dense, dim, p, out);
}

int skml_sparse_encode_bf16(skml_ctx* c, const uint16_t* dense, int64_t dim, const skml_params* p,
                            skml_sparse** out) {
    return encode_dense_x<bf16_t>(c, reinterpret_cast<const bf16_t*>(dense), dim, p, out);
}

int skml_sparse_encode_f16(skml_ctx* c, const uint16_t* dense, int64_t dim, const skml_params* p,
                           skml_sparse** out) {
    return encode_dense_x<f16_t>(c, reinterpret_cast<const f16_t*>(dense), dim, p, out);
}

int skml_sparse_encode_f64(skml_ctx* c, const double* dense, int64_t dim, const skml_params* p,
                           skml_sparse** out) {
    if (!c || !out || dim < 0) return fail(SKML_E_ARG, "bad sparse arguments");
    if (int e = check_params(p)) return e;
    HIP_TRY(hipSetDevice(c->device));
    const size_t cap = (size_t)std::max<int64_t>(dim, 1);
    int32_t* keys = scratch<int32_t>(c, kSlotCKeys, cap);
    double* vals = scratch<double>(c, kSlotCVals, cap);
    if (!keys || !vals) return fail(SKML_E_OOM, "compaction output");
    int64_t nnz = 0;
    if (int e = compact_any<double>(c, dense, dim, keys, vals, &nnz, true)) return e;
    return encode_kv(c, keys, vals, true, nnz, p, out);
}

// ---- standalone DeltaAdaptiveEncoder: one group, no MinMax ----
int skml_delta_encode(skml_ctx* c, const int32_t* keys, int64_t n, int32_t* num_intervals, int32_t* flag_kind,
                      int64_t* n_flag_bits, int64_t* n_delta_bits, uint64_t* flag_words_dev,
                      uint64_t* delta_words_dev, int64_t words_cap) {
    if (!c || !keys || n <= 0 || !num_intervals || !flag_kind || !n_flag_bits || !n_delta_bits)
        return fail(SKML_E_ARG, "bad delta arguments");
    if (n > (int64_t)INT32_MAX) return fail(SKML_E_ARG, "n exceeds Java int");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    skml_sparse tmp;
    tmp.device = c->device;
    tmp.nnz = n;
    SpGroups& G = tmp.g;
    G.G = 1;
    G.rows = 0;
    G.gstart[0] = 0;
    G.gstart[1] = n;
    G.cols[0] = 1;
    uint8_t* need = scratch<uint8_t>(c, kSlotNeed, (size_t)n);
    uint32_t* small = scratch<uint32_t>(c, kSlotSmall, (size_t)kMaxGroups * kDeltaHist + 64);
    const int64_t fwn = flag_words_max(n), dwn = delta_words_max(n);
    const size_t o_w = align_up(sizeof(SpGroups), 256);
    char* blk = static_cast<char*>(ctx_scratch(c, kSlotDeltaEnc, o_w + sizeof(uint64_t) * (size_t)(fwn + dwn)));
    if (!need || !small || !blk) return fail(SKML_E_OOM, "delta scratch");
    tmp.g_dev = reinterpret_cast<SpGroups*>(blk);
    uint64_t* fwd = reinterpret_cast<uint64_t*>(blk + o_w);
    uint64_t* dwd = fwd + fwn;
    int rc = upload_groups(c, &tmp);
    tmp.g_dev = nullptr;  // scratch-owned
    if (rc) return rc;
    SpGroups* g_dev = reinterpret_cast<SpGroups*>(blk);
    HIP_TRY(hipMemsetAsync(small, 0, sizeof(uint32_t) * ((size_t)kMaxGroups * kDeltaHist + 1), st));
    HIP_TRY(launch_group_prep(st, keys, n, g_dev, need, small, small + kMaxGroups * kDeltaHist, nullptr, 0, nullptr,
                              nullptr));
    if (int e = encode_delta_device(c, st, g_dev, keys, need, n, small, small + kMaxGroups * kDeltaHist, fwd, dwd))
        return e;
    if (int e = sync_to_host(c, &G, g_dev, sizeof(SpGroups))) return e;
    if (G.status & kSpOrder) return fail(SKML_E_ORDER, "Log for a non-positive key delta (keys must ascend strictly)");
    *num_intervals = G.m[0];
    *flag_kind = G.kind[0];
    *n_flag_bits = G.fb[1];
    *n_delta_bits = G.db[1];
    const int64_t fw = (G.fb[1] + 63) / 64, dw = (G.db[1] + 63) / 64;
    if (flag_words_dev || delta_words_dev) {
        if (fw > words_cap || dw > words_cap)
            return fail(SKML_E_ARG, "words_cap %lld < needed %lld", (long long)words_cap, (long long)std::max(fw, dw));
        if (flag_words_dev && fw)
            HIP_TRY(hipMemcpyAsync(flag_words_dev, fwd, sizeof(uint64_t) * fw, hipMemcpyDeviceToDevice, st));
        if (delta_words_dev && dw)
            HIP_TRY(hipMemcpyAsync(delta_words_dev, dwd, sizeof(uint64_t) * dw, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SKML_OK;
}

int skml_delta_decode(skml_ctx* c, int64_t n, int32_t num_intervals, int32_t flag_kind, const uint64_t* flag_words,
                      int64_t n_flag_words, const uint64_t* delta_words, int64_t n_delta_words, int32_t* keys_dev) {
    if (!c || n <= 0 || !keys_dev || !(num_intervals == 1 || num_intervals == 2 || num_intervals == 4 ||
                                       num_intervals == 8 || num_intervals == 16))
        return fail(SKML_E_ARG, "bad delta decode arguments");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    skml_sparse tmp;
    tmp.device = c->device;
    tmp.nnz = n;
    SpGroups& G = tmp.g;
    G.G = 1;
    G.gstart[0] = 0;
    G.gstart[1] = n;
    G.m[0] = num_intervals;
    G.kind[0] = flag_kind ? 1 : 0;
    G.fb[0] = 0;
    G.fb[1] = n_flag_words * 64;  // trailing zero words were trimmed by toLongArray
    G.db[0] = 0;
    G.db[1] = n_delta_words * 64;
    // toLongArray may trim to zero words; keep readable (zero) words behind the caller's streams
    const int64_t nfw = std::max<int64_t>(n_flag_words, 0), ndw = std::max<int64_t>(n_delta_words, 0);
    tmp.flag_words = const_cast<uint64_t*>(flag_words);
    tmp.delta_words = const_cast<uint64_t*>(delta_words);
    tmp.n_flag_words = nfw;
    tmp.n_delta_words = ndw;
    int32_t* gb = scratch<int32_t>(c, kSlotGBins, (size_t)n);
    if (!gb) return fail(SKML_E_OOM, "delta scratch");
    if (hipMalloc(&tmp.g_dev, sizeof(SpGroups)) != hipSuccess) return fail(SKML_E_OOM, "group table");
    int rc = upload_groups(c, &tmp);
    if (!rc) rc = decode_groups(c, &tmp, keys_dev, gb, false);
    (void)hipStreamSynchronize(st);
    (void)hipFree(tmp.g_dev);
    tmp.g_dev = nullptr;
    tmp.flag_words = tmp.delta_words = nullptr;  // caller-owned
    return rc;
}

}  // extern "C"
