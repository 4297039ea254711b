// skml_dense_api.cpp -- host side of the dense codecs of the C ABI (include/skml.h): the
// QuantileQuantizer (quantize, parallelQuantize and its sharded form, batches) and the
// UniformQuantizer in fp32 / fp64 / 16-bit storage, their workspaces and launch planning, decode
// and decode-sum.
#include <algorithm>
#include <cstring>
#include <vector>

#include "skml_host.hpp"

using namespace skml;

namespace {

size_t ws_layout(int64_t chunks, Workspace* w, char* base) {
    const int64_t nwg = (chunks + kLeafChunks - 1) / kLeafChunks;
    const int64_t full = chunks / kLeafChunks;
    const int64_t up = (full >> kMergeGroupLog) + 2 * kMaxLevels + 8;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return base ? (void*)(base + o) : nullptr;
    };
    Workspace t;
    t.done = (unsigned*)take(256);
    t.part = (LeafPartial*)take(sizeof(LeafPartial) * (size_t)(nwg + 1));
    t.nodes6 = (float*)take(sizeof(float) * kK * (size_t)(full + 1));
    t.roots = (float*)take(sizeof(float) * kK * kMaxLevels);
    t.upA = (float*)take(sizeof(float) * kK * (size_t)up);
    t.upB = (float*)take(sizeof(float) * kK * (size_t)up);
    t.raw = (double*)take(sizeof(double) * SKML_MAX_BINS);
    t.lut = (QuantLut*)take(sizeof(QuantLut));
    t.uni = (UniPartial*)take(sizeof(UniPartial) * kUniMaxParts);
    t.qflags = (int*)take(sizeof(int) * 4);
    t.ubits = (uint8_t*)take((size_t)upper_node_count(full * kLeafChunks) + 64);
    t.part_red = (LeafPartial*)take(sizeof(LeafPartial) * (size_t)(full + 8));
    if (w) *w = t;
    return off;
}

}  // namespace

int skml::ensure_ws(skml_ctx* ctx, int64_t chunks, Workspace* w) {
    const size_t need = ws_layout(chunks, nullptr, nullptr);
    bool grew;
    if (int st = reserve(ctx, ctx->ws, need, need + need / 4, "dense workspace", &grew)) return st;
    // the fused summary's arrival counter starts at 0; zeroed on the context's own stream: a
    // hipMemset goes to the null stream, which a non-blocking stream (the batch encode's side
    // lane) does not wait for, so a fresh side workspace could be counted on before it was
    // zeroed and the summary skipped (a payload without a header, tests/test_gpu_configs.py C4)
    if (grew) HIP_TRY(hipMemsetAsync(ctx->ws.p, 0, 256, ctx->stream));
    ws_layout(chunks, w, (char*)ctx->ws.p);
    return SKML_OK;
}

namespace {

struct Workspace64 {
    LeafPartial64* part;
    double* nodes6;
    double* roots;
    double* upA;
    double* upB;
    double* raw;
    uint8_t* ubits;
};

size_t ws64_layout(int64_t chunks, Workspace64* w, char* base) {
    const int64_t tiles = (chunks + kLeafChunks - 1) / kLeafChunks;
    const int64_t up = (tiles >> 3) + 8;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return base ? (void*)(base + o) : nullptr;
    };
    Workspace64 t;
    t.part = (LeafPartial64*)take(sizeof(LeafPartial64) * (size_t)(tiles + 1));
    t.nodes6 = (double*)take(sizeof(double) * kK * (size_t)(tiles + 1));
    t.roots = (double*)take(sizeof(double) * kK * kMaxLevels);
    t.upA = (double*)take(sizeof(double) * kK * (size_t)up);
    t.upB = (double*)take(sizeof(double) * kK * (size_t)up);
    t.raw = (double*)take(sizeof(double) * SKML_MAX_BINS);
    t.ubits = (uint8_t*)take((size_t)upper_node_count(tiles * kLeafChunks) + 64);
    if (w) *w = t;
    return off;
}

int ensure_ws_f64(skml_ctx* ctx, int64_t chunks, Workspace64* w) {
    const size_t need = ws64_layout(chunks, nullptr, nullptr);
    if (int st = reserve(ctx, ctx->ws64, need, need + need / 4, "fp64 sketch workspace")) return st;
    ws64_layout(chunks, w, (char*)ctx->ws64.p);
    return SKML_OK;
}

int64_t* ranks_of(const skml_ctx* c) { return static_cast<int64_t*>(c->ranks.p); }

// getQuantiles(int) ranks: curFrac accumulated by repeated `+= 1/B` in double
// (HeapQuantileSketch.java:304-321); depends only on (n, B) so it is planned on the host.
int ensure_ranks(skml_ctx* ctx, int64_t n, int bins) {
    if (ctx->ranks_n == n && ctx->ranks_bins == bins) return SKML_OK;
    const size_t bytes = sizeof(int64_t) * (size_t)bins;  // bins - 1 ranks and one spare
    if (int st = reserve(ctx, ctx->ranks, bytes, bytes, "rank table")) return st;
    // written on the stream ahead of the sketch (no host table, no synchronisation); the kernels
    // reading it follow on the same stream
    HIP_TRY(launch_set_ranks(ctx->stream, n, bins, ranks_of(ctx)));
    ctx->ranks_n = n;
    ctx->ranks_bins = bins;
    return SKML_OK;
}

// Plan the upper merge passes for the trees of bits >= 6 of the chunk count.
struct Tree {
    int level;           // tree level l (bit of chunks)
    int m;               // remaining log2 node count
    int cur_level;       // level of its current nodes
    int64_t src;         // first node index in the current src buffer
    int64_t chunk_base;  // first chunk
};

}  // namespace

extern "C" {

int skml_debug_leaf_stage(skml_ctx* c, const float* x, int64_t n, int stage, int iters,
                          double* avg_ms) {
    if (!c || !x || n < kChunk || iters < 1 || !avg_ms) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t chunks = n / kChunk;
    Workspace w;
    int st = ensure_ws(c, chunks, &w);
    if (st) return st;
    const int64_t nwg = (chunks + kLeafChunks - 1) / kLeafChunks;
    const size_t stage_bytes = sizeof(float) * 512 * (size_t)nwg;
    if ((st = reserve(c, c->stage, stage_bytes, stage_bytes, "stage buffer"))) return st;
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(launch_leaf_stage(c->stream, stage, x, chunks, 12345, c->jump_tab, w.part,
                              (float*)c->stage.p, w.roots));
    HIP_TRY(hipEventRecord(a, c->stream));
    for (int i = 0; i < iters; i++)
        HIP_TRY(launch_leaf_stage(c->stream, stage, x, chunks, 12345, c->jump_tab, w.part,
                                  (float*)c->stage.p, w.roots));
    HIP_TRY(hipEventRecord(b, c->stream));
    HIP_TRY(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *avg_ms = ms / iters;
    return SKML_OK;
}

size_t skml_dense_payload_bytes(int64_t n, int32_t bin_num) {
    if (n < 0 || bin_num < 2 || bin_num > SKML_MAX_BINS) return 0;
    const size_t rounded = align_up((size_t)n, 1024);
    return dense_codes_offset(bin_num) + align_up(rounded * (size_t)code_bits_for(bin_num) / 8, 256);
}

static int check_dense_args(skml_ctx* c, const void* x, int64_t n, int bins, const void* payload,
                            size_t cap) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (n < 0 || n > 0x7FFFFFFFLL) return fail(SKML_E_ARG, "n=%lld outside Java int range", (long long)n);
    if (bins < 2 || bins > SKML_MAX_BINS)
        return fail(SKML_E_ARG, "Invalid partition number: %d", bins);  // QSketchUtils.java:40-43
    if (n > 0 && (!x || ((uintptr_t)x) % 16 != 0))
        return fail(SKML_E_ARG, "input must be a 16-byte aligned device pointer");
    if (!valid_payload_ptr(payload)) return fail(SKML_E_ARG, "payload must be 256-byte aligned");
    if (cap < skml_dense_payload_bytes(n, bins))
        return fail(SKML_E_ARG, "payload capacity %zu < %zu", cap, skml_dense_payload_bytes(n, bins));
    return SKML_OK;
}

}  // extern "C"

namespace {
// Upper merge passes for the trees of bits l >= 7 of the chunk count (bit 6 is a single leaf
// node): each pass merges up to 2^kMergeGroupLog nodes of a tree per workgroup.
std::vector<MergePass> plan_merge_passes(int64_t chunks) {
    std::vector<Tree> trees;
    for (int l = kMaxLevels - 1; l > kLeafTopLevel; l--) {
        if (!((chunks >> l) & 1)) continue;
        Tree t;
        t.level = l;
        t.m = l - kLeafTopLevel;
        t.cur_level = kLeafTopLevel;
        t.chunk_base = (chunks >> (l + 1)) << (l + 1);
        t.src = t.chunk_base >> kLeafTopLevel;
        trees.push_back(t);
    }
    std::vector<MergePass> passes;
    while (true) {
        MergePass pass;
        std::memset(&pass, 0, sizeof(pass));
        int64_t dst_off = 0;
        int wg = 0;
        for (auto& t : trees) {
            if (t.m == 0) continue;
            const int g = t.m < kMergeGroupLog ? t.m : kMergeGroupLog;
            MergeJob& j = pass.job[pass.njobs];
            j.src_node = t.src;
            j.dst_node = dst_off;
            j.chunk_base = t.chunk_base;
            j.level_in = t.cur_level;
            j.group_log = g;
            j.groups = 1 << (t.m - g);
            j.root_level = (t.m - g == 0) ? t.level : -1;
            pass.wg_prefix[pass.njobs] = wg;
            wg += j.groups;
            pass.njobs++;
            t.src = dst_off;
            dst_off += j.groups;
            t.m -= g;
            t.cur_level += g;
        }
        if (pass.njobs == 0) break;
        pass.wg_prefix[pass.njobs] = wg;
        passes.push_back(pass);
    }
    return passes;
}
// a final pass of at most kFuseMaxWg workgroup-merges runs inside the previous pass's last
// workgroup, one merge after another (sizes that are not 64^k chunks end with a few small trees:
// C3's 26.8 M values leave 2, which otherwise cost a launch of their own)
constexpr int kFuseMaxWg = 4;
bool fuse_next_pass(const std::vector<MergePass>& passes, size_t i) {
    return i + 2 == passes.size() && passes[i + 1].wg_prefix[passes[i + 1].njobs] <= kFuseMaxWg;
}
}  // namespace

namespace {
// The sketch of x[0, n): leaf + upper merge passes.  summary: the last pass's last workgroup
// also runs the summary into `payload` (returns *fused = true); otherwise the levels stay in
// w.roots and the partials in w.part for a caller-side summary or a SketchRecord.
int run_sketch_f32(skml_ctx* c, const void* x, int64_t n, uint64_t s0, const Workspace& w, const skml_params* p,
                   void* payload, bool summary, bool* fused_out, int xtype = kXF32) {
    const int64_t chunks = n / kChunk;
    const int64_t nwg = (chunks + kLeafChunks - 1) / kLeafChunks;  // leaf partials (one per wave tile)
    bool fused = false;
    if (chunks > 0) {
        {
            KernelTimer kt(c, SKML_K_LEAF);
            HIP_TRY(launch_leaf(c->stream, x, chunks, s0, c->jump_tab, w.part, w.nodes6, w.roots, w.ubits, xtype));
        }
        if (c->after_leaf) {
            HIP_TRY(hipEventRecord(c->after_leaf, c->stream));
            c->after_leaf = nullptr;
        }
        std::vector<MergePass> passes = plan_merge_passes(chunks);
        if (summary && !passes.empty()) passes.back().fuse_summary = 1;
        // the first pass reduces the leaf partials of the tiles it merges (every tile of the
        // trees of level >= 7: [0, 2 * (chunks >> 7))) for the summary, one per workgroup
        const int64_t nred = passes.empty() ? 0 : passes[0].wg_prefix[passes[0].njobs];
        const int64_t part_from = passes.empty() ? 0 : (chunks >> 7) << 1;
        const float* src = w.nodes6;
        float* dst = w.upA;
        for (size_t i = 0; i < passes.size(); i++) {
            const bool fuse_next = fuse_next_pass(passes, i);
            float* next_dst = (dst == w.upA) ? w.upB : w.upA;
            KernelTimer kt(c, SKML_K_MERGE);
            HIP_TRY(launch_merge_pass(c->stream, passes[i], fuse_next ? &passes[i + 1] : nullptr, src, dst, next_dst,
                                      w.roots, s0, c->jump_tab, w.done, x, n, w.part, nwg, ranks_of(c), p->bin_num,
                                      p->dedup ? 1 : 0, payload, w.raw, summary_lut(w.lut), w.ubits,
                                      summary ? w.part_red : nullptr, summary ? nred : 0, summary ? part_from : 0,
                                      xtype));
            src = dst;
            dst = next_dst;
            if (fuse_next) break;
        }
        fused = summary && !passes.empty();
    }
    *fused_out = fused;
    return SKML_OK;
}

// java.util.Random state after k more draws (affine jump-ahead by squaring)
uint64_t lcg_skip(uint64_t s, uint64_t k) {
    uint64_t a = kLcgMult, c = kLcgAdd;
    while (k) {
        if (k & 1) s = (a * s + c) & kLcgMask;
        c = (a * c + c) & kLcgMask;
        a = (a * a) & kLcgMask;
        k >>= 1;
    }
    return s;
}
// Random draws of one sketch over n updates: chunk c's leaf compaction plus its carries,
// sum over c < C of (1 + trailing_ones(c)) = 2C - popcount(C).
uint64_t sketch_draws(int64_t n) {
    const uint64_t C = (uint64_t)(n / kChunk);
    return 2 * C - (uint64_t)__builtin_popcountll(C);
}
}  // namespace

// QuantileQuantizer.quantize of x in storage type xtype: the sketch and the quantize pass widen a
// 16-bit input in registers, everything else is the fp32 encode.
static int dense_encode_x(skml_ctx* c, const void* x, int xtype, int64_t n, const skml_params* p, void* payload,
                          size_t cap) {
    skml_params def;
    p = params_or_default(p, &def, /*clear_dedup=*/false);
    int st = check_dense_args(c, x, n, p->bin_num, payload, cap);
    if (st) return st;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t chunks = n / kChunk;
    Workspace w;
    if ((st = ensure_ws(c, chunks, &w))) return st;
    if ((st = ensure_ranks(c, n, p->bin_num))) return st;
    const uint64_t s0 = ((uint64_t)p->seed ^ kLcgMult) & kLcgMask;
    const int64_t nwg = (chunks + kLeafChunks - 1) / kLeafChunks;
    bool fused = false;
    if ((st = run_sketch_f32(c, x, n, s0, w, p, payload, true, &fused, xtype))) return st;
    if (!fused) {
        KernelTimer kt(c, SKML_K_SUMMARY);
        HIP_TRY(launch_summary(c->stream, x, n, w.part, nwg, w.roots, ranks_of(c), p->bin_num,
                               p->dedup ? 1 : 0, payload, w.raw, summary_lut(w.lut), xtype));
    }
    {
        KernelTimer kt(c, SKML_K_QUANTIZE);
        HIP_TRY(launch_quantize(c->stream, &c->qres, x, n, payload, summary_lut(w.lut), p->bin_num, xtype));
    }
    return SKML_OK;
}

extern "C" {

int skml_dense_encode_f32(skml_ctx* c, const float* x, int64_t n, const skml_params* p,
                          void* payload, size_t cap) {
    return dense_encode_x(c, x, kXF32, n, p, payload, cap);
}

int skml_dense_encode_bf16(skml_ctx* c, const uint16_t* x, int64_t n, const skml_params* p,
                           void* payload, size_t cap) {
    return dense_encode_x(c, x, kXBF16, n, p, payload, cap);
}

int skml_dense_encode_f16(skml_ctx* c, const uint16_t* x, int64_t n, const skml_params* p,
                          void* payload, size_t cap) {
    return dense_encode_x(c, x, kXF16, n, p, payload, cap);
}

}  // extern "C"

namespace {
// fp64 sketch of x[0, n): leaf + per-tree merge passes; levels in w.roots, partials in w.part.
int run_sketch_f64(skml_ctx* c, const double* x, int64_t n, uint64_t s0, const Workspace64& w) {
    const int64_t chunks = n / kChunk;
    {
        KernelTimer kt(c, SKML_K_LEAF);
        HIP_TRY(launch_leaf2_f64(c->stream, x, chunks, s0, c->jump_tab, w.part, w.nodes6, w.roots, w.ubits));
    }
    // upper trees: the fp32 pass plan over double nodes (k_merge64)
    const std::vector<MergePass> passes = plan_merge_passes(chunks);
    Workspace wq;  // for its self-resetting arrival counter
    if (int st = ensure_ws(c, 0, &wq)) return st;
    const double* src = w.nodes6;
    double* dst = w.upA;
    for (size_t i = 0; i < passes.size(); i++) {
        const bool fuse_next = fuse_next_pass(passes, i);
        double* next_dst = (dst == w.upA) ? w.upB : w.upA;
        KernelTimer kt(c, SKML_K_MERGE);
        HIP_TRY(launch_merge_pass64(c->stream, passes[i], fuse_next ? &passes[i + 1] : nullptr, src, dst, next_dst,
                                    w.roots, s0, c->jump_tab, wq.done, w.ubits,
                                    (chunks / kLeafChunks) * kLeafChunks));
        src = dst;
        dst = next_dst;
        if (fuse_next) break;
    }
    return SKML_OK;
}

// What the fp32 and fp64 forms of parallelQuantize and of the UniformQuantizer differ in: the
// record and partial types, the sketch workspace and the launch wrappers.
template <typename T> struct SketchT;
template <> struct SketchT<float> {
    using Record = SketchRecord;
    using Partial = LeafPartial;
    using Ws = Workspace;
    static int ws(skml_ctx* c, int64_t chunks, Ws* w) { return ensure_ws(c, chunks, w); }
    static int lut(skml_ctx*, const Ws& w, QuantLut** lut) {
        *lut = summary_lut(w.lut);  // none: the quantize pass builds its own table
        return SKML_OK;
    }
    static int sketch(skml_ctx* c, const float* x, int64_t n, uint64_t s0, const Ws& w) {
        skml_params p;
        skml_params_default(&p);
        bool fused = false;
        return run_sketch_f32(c, x, n, s0, w, &p, nullptr, false, &fused);
    }
    static hipError_t record(hipStream_t st, const float* x, int64_t n, const Ws& w, int64_t nparts, Record* rec) {
        return launch_sketch_record(st, x, n, w.part, nparts, w.roots, rec);
    }
    // the records' merge and the merged sketch's summary are one launch
    static hipError_t merge_summary(skml_ctx* c, const Record* recs, int nrec, uint64_t s0, uint64_t draws_all,
                                    int64_t n_total, int64_t n, const skml_params* p, void* payload, const Ws& w,
                                    QuantLut* lut, float* roots, float* tail, Partial* part) {
        return launch_sketch_merge(c->stream, recs, nrec, s0, draws_all, c->jump_tab, n_total, n, ranks_of(c),
                                   p->bin_num, p->dedup ? 1 : 0, payload, w.raw, lut, roots, tail, part);
    }
    static hipError_t uniform(hipStream_t st, const float* x, int64_t n, int bins, const Workspace& w, void* payload) {
        return launch_uniform(st, x, n, bins, w.uni, payload, w.lut, w.qflags);
    }
    static hipError_t quantize(skml_ctx* c, const float* x, int64_t n, void* payload, const QuantLut* lut,
                               const int*, int bins) {
        return launch_quantize(c->stream, &c->qres, x, n, payload, lut, bins);
    }
};
template <> struct SketchT<double> {
    using Record = SketchRecord64;
    using Partial = LeafPartial64;
    using Ws = Workspace64;
    static int ws(skml_ctx* c, int64_t chunks, Ws* w) { return ensure_ws_f64(c, chunks, w); }
    static int lut(skml_ctx* c, const Ws&, QuantLut** lut) {
        Workspace wq;  // the quantize LUT lives in the fp32 workspace
        if (int st = ensure_ws(c, 0, &wq)) return st;
        *lut = wq.lut;
        return SKML_OK;
    }
    static int sketch(skml_ctx* c, const double* x, int64_t n, uint64_t s0, const Ws& w) {
        return run_sketch_f64(c, x, n, s0, w);
    }
    static hipError_t record(hipStream_t st, const double* x, int64_t n, const Ws& w, int64_t nparts, Record* rec) {
        return launch_sketch_record64(st, x, n, w.part, nparts, w.roots, rec);
    }
    static hipError_t merge_summary(skml_ctx* c, const Record* recs, int nrec, uint64_t s0, uint64_t draws_all,
                                    int64_t n_total, int64_t n, const skml_params* p, void* payload, const Ws& w,
                                    QuantLut* lut, double* roots, double* tail, Partial* part) {
        const hipError_t e = launch_sketch_merge64(c->stream, recs, nrec, s0, draws_all, c->jump_tab, roots, tail, part);
        if (e != hipSuccess) return e;
        return launch_summary64(c->stream, nullptr, n_total, part, nrec, roots, ranks_of(c), p->bin_num,
                                p->dedup ? 1 : 0, payload, w.raw, lut, tail, 1, n);
    }
    static hipError_t uniform(hipStream_t st, const double* x, int64_t n, int bins, const Workspace& w, void* payload) {
        return launch_uniform64(st, x, n, bins, w.uni, payload, w.lut, w.qflags);
    }
    static hipError_t quantize(skml_ctx* c, const double* x, int64_t n, void* payload, const QuantLut* lut,
                               const int* qflags, int bins) {
        return launch_quantize64(c->stream, x, n, payload, lut, qflags, bins);
    }
};

// parallelQuantize's scratch in the context's record buffer: the caller's own slice records (the
// parallel path; none for the sharded one), then the merged sketch's levels, its tail and the
// records' partials.
template <typename T>
struct RecScratch {
    typename SketchT<T>::Record* recs;
    T* roots;
    T* tail;
    typename SketchT<T>::Partial* part;
};
template <typename T>
int ensure_sk(skml_ctx* c, int nrec_own, int nrec, RecScratch<T>* out) {
    const size_t rec_bytes = align_up(sizeof(typename SketchT<T>::Record) * (size_t)nrec_own, 256);
    const size_t roots_bytes = align_up(sizeof(T) * kMaxLevels * kK, 256);
    const size_t tail_bytes = align_up(sizeof(T) * kChunk, 256);
    const size_t need = rec_bytes + roots_bytes + tail_bytes + sizeof(typename SketchT<T>::Partial) * (size_t)nrec;
    if (int st = reserve(c, c->sk, need, need, "sketch scratch")) return st;
    uint8_t* b = static_cast<uint8_t*>(c->sk.p);
    out->recs = reinterpret_cast<typename SketchT<T>::Record*>(b);
    out->roots = reinterpret_cast<T*>(b + rec_bytes);
    out->tail = reinterpret_cast<T*>(b + rec_bytes + roots_bytes);
    out->part = reinterpret_cast<typename SketchT<T>::Partial*>(b + rec_bytes + roots_bytes + tail_bytes);
    return SKML_OK;
}

int check_shards(const int64_t* shard_n, int32_t nshards, int32_t shard, int64_t n, int64_t* total,
                 uint64_t* draws_before, uint64_t* draws_all) {
    if (!shard_n || nshards < 1 || shard < 0 || shard >= nshards)
        return fail(SKML_E_ARG, "bad shard table (nshards=%d shard=%d)", nshards, shard);
    int64_t tot = 0;
    uint64_t before = 0, all = 0;
    for (int i = 0; i < nshards; i++) {
        if (shard_n[i] < 0) return fail(SKML_E_ARG, "shard %d has %lld values", i, (long long)shard_n[i]);
        tot += shard_n[i];
        if (tot > 0x7FFFFFFFLL) return fail(SKML_E_ARG, "total n=%lld outside Java int range", (long long)tot);
        if (i < shard) before += sketch_draws(shard_n[i]);
        all += sketch_draws(shard_n[i]);
    }
    if (shard_n[shard] != n)
        return fail(SKML_E_ARG, "shard %d: n=%lld but the table says %lld", shard, (long long)n,
                    (long long)shard_n[shard]);
    *total = tot;
    *draws_before = before;
    *draws_all = all;
    return SKML_OK;
}

// Sketch x[0, n) with draws starting after `skip` draws of Random(seed) into rec.
template <typename T>
int sketch_into_record(skml_ctx* c, const T* x, int64_t n, int64_t seed, uint64_t skip,
                       typename SketchT<T>::Record* rec) {
    const int64_t chunks = n / kChunk;
    typename SketchT<T>::Ws w;
    int st = SketchT<T>::ws(c, chunks, &w);
    if (st) return st;
    const uint64_t s0 = lcg_skip(((uint64_t)seed ^ kLcgMult) & kLcgMask, skip);
    if ((st = SketchT<T>::sketch(c, x, n, s0, w))) return st;
    KernelTimer kt(c, SKML_K_SUMMARY);
    HIP_TRY(SketchT<T>::record(c->stream, x, n, w, (chunks + kLeafChunks - 1) / kLeafChunks, rec));
    return SKML_OK;
}

// Merge nrec records, summary of n_total values, quantize x[0, n).
template <typename T>
int merge_and_quantize(skml_ctx* c, const T* x, int64_t n, const typename SketchT<T>::Record* recs, int nrec,
                       int64_t n_total, uint64_t draws_all, const skml_params* p, void* payload,
                       const RecScratch<T>& sk) {
    typename SketchT<T>::Ws w;
    int st = SketchT<T>::ws(c, n / kChunk, &w);
    if (st) return st;
    QuantLut* lut;
    if ((st = SketchT<T>::lut(c, w, &lut))) return st;
    if ((st = ensure_ranks(c, n_total, p->bin_num))) return st;
    const uint64_t s0 = ((uint64_t)p->seed ^ kLcgMult) & kLcgMask;
    {
        KernelTimer kt(c, SKML_K_SUMMARY);
        HIP_TRY(SketchT<T>::merge_summary(c, recs, nrec, s0, draws_all, n_total, n, p, payload, w, lut, sk.roots,
                                          sk.tail, sk.part));
    }
    KernelTimer kt(c, SKML_K_QUANTIZE);
    HIP_TRY(SketchT<T>::quantize(c, x, n, payload, lut, nullptr, p->bin_num));
    return SKML_OK;
}

template <typename T>
int sketch_shard(skml_ctx* c, const T* x, int64_t n, const int64_t* shard_n, int32_t nshards, int32_t shard,
                 int64_t seed, void* record_dev) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (n > 0 && (!x || ((uintptr_t)x) % 16 != 0))
        return fail(SKML_E_ARG, "input must be a 16-byte aligned device pointer");
    if (!record_dev || ((uintptr_t)record_dev) % 16 != 0)
        return fail(SKML_E_ARG, "record must be a 16-byte aligned device pointer");
    int64_t total;
    uint64_t before, all;
    int st = check_shards(shard_n, nshards, shard, n, &total, &before, &all);
    if (st) return st;
    HIP_TRY(hipSetDevice(c->device));
    return sketch_into_record<T>(c, x, n, seed, before, static_cast<typename SketchT<T>::Record*>(record_dev));
}

template <typename T>
int encode_sharded(skml_ctx* c, const T* x, int64_t n, const int64_t* shard_n, int32_t nshards, int32_t shard,
                   const void* records_dev, const skml_params* p, void* payload, size_t cap) {
    skml_params def;
    p = params_or_default(p, &def, /*clear_dedup=*/true);
    int st = check_dense_args(c, x, n, p->bin_num, payload, cap);
    if (st) return st;
    if (!records_dev || ((uintptr_t)records_dev) % 16 != 0)
        return fail(SKML_E_ARG, "records must be a 16-byte aligned device pointer");
    int64_t total;
    uint64_t before, all;
    if ((st = check_shards(shard_n, nshards, shard, n, &total, &before, &all))) return st;
    HIP_TRY(hipSetDevice(c->device));
    RecScratch<T> sk;
    if ((st = ensure_sk(c, 0, nshards, &sk))) return st;
    return merge_and_quantize<T>(c, x, n, static_cast<const typename SketchT<T>::Record*>(records_dev), nshards, total,
                                 all, p, payload, sk);
}

template <typename T>
int encode_parallel(skml_ctx* c, const T* x, int64_t n, int32_t threads, const skml_params* p, void* payload,
                    size_t cap) {
    skml_params def;
    p = params_or_default(p, &def, /*clear_dedup=*/true);
    int st = check_dense_args(c, x, n, p->bin_num, payload, cap);
    if (st) return st;
    if (threads < 1 || threads > 65536) return fail(SKML_E_ARG, "Invalid parallelism: %d", threads);
    HIP_TRY(hipSetDevice(c->device));
    // QuantileQuantizer.java:66-68: thread t takes [t*(n/T), ...), the last one the remainder
    std::vector<int64_t> shard_n((size_t)threads, n / threads);
    shard_n.back() = n - (int64_t)(threads - 1) * (n / threads);
    RecScratch<T> sk;
    if ((st = ensure_sk(c, threads, threads, &sk))) return st;
    uint64_t skip = 0;
    for (int t = 0; t < threads; t++) {
        const T* xt = x + (int64_t)t * (n / threads);
        if ((st = sketch_into_record<T>(c, xt, shard_n[t], p->seed, skip, sk.recs + t))) return st;
        skip += sketch_draws(shard_n[t]);
    }
    return merge_and_quantize<T>(c, x, n, sk.recs, threads, n, skip, p, payload, sk);
}

template <typename T>
int encode_uniform(skml_ctx* c, const T* x, int64_t n, const skml_params* p, void* payload, size_t cap) {
    skml_params def;
    p = params_or_default(p, &def, /*clear_dedup=*/false);
    int st = check_dense_args(c, x, n, p->bin_num, payload, cap);
    if (st) return st;
    HIP_TRY(hipSetDevice(c->device));
    Workspace w;
    if ((st = ensure_ws(c, 0, &w))) return st;
    {
        KernelTimer kt(c, SKML_K_SUMMARY);
        HIP_TRY(SketchT<T>::uniform(c->stream, x, n, p->bin_num, w, payload));
    }
    {
        KernelTimer kt(c, SKML_K_QUANTIZE);
        HIP_TRY(SketchT<T>::quantize(c, x, n, payload, w.lut, w.qflags, p->bin_num));
    }
    return SKML_OK;
}

}  // namespace

extern "C" {

size_t skml_sketch_record_bytes(int32_t fp64) { return fp64 ? sizeof(SketchRecord64) : sizeof(SketchRecord); }

int skml_dense_sketch_shard_f32(skml_ctx* c, const float* x, int64_t n, const int64_t* shard_n, int32_t nshards,
                                int32_t shard, int64_t seed, void* record_dev) {
    return sketch_shard<float>(c, x, n, shard_n, nshards, shard, seed, record_dev);
}

int skml_dense_sketch_shard_f64(skml_ctx* c, const double* x, int64_t n, const int64_t* shard_n, int32_t nshards,
                                int32_t shard, int64_t seed, void* record_dev) {
    return sketch_shard<double>(c, x, n, shard_n, nshards, shard, seed, record_dev);
}

int skml_dense_encode_sharded_f32(skml_ctx* c, const float* x, int64_t n, const int64_t* shard_n, int32_t nshards,
                                  int32_t shard, const void* records_dev, const skml_params* p, void* payload,
                                  size_t cap) {
    return encode_sharded<float>(c, x, n, shard_n, nshards, shard, records_dev, p, payload, cap);
}

int skml_dense_encode_sharded_f64(skml_ctx* c, const double* x, int64_t n, const int64_t* shard_n, int32_t nshards,
                                  int32_t shard, const void* records_dev, const skml_params* p, void* payload,
                                  size_t cap) {
    return encode_sharded<double>(c, x, n, shard_n, nshards, shard, records_dev, p, payload, cap);
}

int skml_dense_encode_parallel_f32(skml_ctx* c, const float* x, int64_t n, int32_t threads, const skml_params* p,
                                   void* payload, size_t cap) {
    return encode_parallel<float>(c, x, n, threads, p, payload, cap);
}

int skml_dense_encode_parallel_f64(skml_ctx* c, const double* x, int64_t n, int32_t threads, const skml_params* p,
                                   void* payload, size_t cap) {
    return encode_parallel<double>(c, x, n, threads, p, payload, cap);
}

int skml_dense_encode_uniform_f32(skml_ctx* c, const float* x, int64_t n, const skml_params* p, void* payload,
                                  size_t cap) {
    return encode_uniform<float>(c, x, n, p, payload, cap);
}

int skml_dense_encode_uniform_f64(skml_ctx* c, const double* x, int64_t n, const skml_params* p, void* payload,
                                  size_t cap) {
    return encode_uniform<double>(c, x, n, p, payload, cap);
}

// Independent buckets, alternately on the caller's stream and a side stream: bucket i+1's
// VALU-bound leaf runs beside bucket i's HBM-bound quantize pass (and its latency-bound merge),
// which a single stream serialises.  Ordered after earlier work on ctx's stream; ctx's stream
// waits for all buckets.  (Forking both lanes off the caller's stream with events measured no
// overlap at all when that stream is the legacy null stream.)
int skml_dense_encode_batch_f32(skml_ctx* c, int32_t nbuckets, const float* const* xs, const int64_t* ns,
                                const skml_params* p, void* const* payloads, const size_t* caps) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (nbuckets < 0 || (nbuckets > 0 && (!xs || !ns || !payloads || !caps)))
        return fail(SKML_E_ARG, "bad bucket arrays (nbuckets=%d)", nbuckets);
    if (nbuckets == 0) return SKML_OK;
    skml_params def;
    p = params_or_default(p, &def, /*clear_dedup=*/false);
    for (int i = 0; i < nbuckets; i++) {
        int st = check_dense_args(c, xs[i], ns[i], p->bin_num, payloads[i], caps[i]);
        if (st) return st;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (nbuckets == 1) return skml_dense_encode_f32(c, xs[0], ns[0], p, payloads[0], caps[0]);
    // Lane 0 is the caller's stream itself; lane 1 is the side context (ensure_side).
    if (int st = ensure_side(c)) return st;
    if (!c->ev_leaf) HIP_TRY(hipEventCreateWithFlags(&c->ev_leaf, hipEventDisableTiming));
    skml_ctx* lane[2] = {c, c->side};
    // lane 1 starts when bucket 0's sketch pass is done (which also orders it after earlier work
    // on the caller's stream), so the lanes stay half a bucket apart: each lane's leaf runs
    // beside the other lane's merge and quantize
    c->after_leaf = c->ev_leaf;
    for (int i = 0; i < nbuckets; i++) {
        if (i == 1) HIP_TRY(hipStreamWaitEvent(lane[1]->stream, c->ev_leaf, 0));
        int st = skml_dense_encode_f32(lane[i & 1], xs[i], ns[i], p, payloads[i], caps[i]);
        if (st) {
            c->after_leaf = nullptr;
            if (i >= 1) {  // lane 1 holds queued buckets: the caller's stream must still wait for them
                (void)hipEventRecord(c->ev_join, c->side->stream);
                (void)hipStreamWaitEvent(c->stream, c->ev_join, 0);
            }
            return st;
        }
        if (i == 0 && c->after_leaf) {  // bucket 0 had no leaf (n < 256): order lane 1 after it
            c->after_leaf = nullptr;
            HIP_TRY(hipEventRecord(c->ev_leaf, c->stream));
        }
    }
    HIP_TRY(hipEventRecord(c->ev_join, c->side->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return SKML_OK;
}

int skml_dense_encode_with_splits_f32(skml_ctx* c, const float* x, int64_t n, const double* splits,
                                      int32_t nsplits, double mn, double mx, void* payload,
                                      size_t cap) {
    int st = check_dense_args(c, x, n, nsplits + 1, payload, cap);
    if (st) return st;
    if (!splits) return fail(SKML_E_ARG, "splits is NULL");
    for (int i = 1; i < nsplits; i++)
        if (!(splits[i - 1] <= splits[i])) return fail(SKML_E_ARG, "splits must be ascending");
    HIP_TRY(hipSetDevice(c->device));
    const size_t stage_bytes = sizeof(double) * (size_t)nsplits;
    if ((st = reserve(c, c->stage, stage_bytes, stage_bytes, "stage buffer"))) return st;
    HIP_TRY(hipMemcpyAsync(c->stage.p, splits, stage_bytes, hipMemcpyHostToDevice, c->stream));
    Workspace w;
    if ((st = ensure_ws(c, 0, &w))) return st;
    HIP_TRY(launch_set_splits(c->stream, payload, n, (const double*)c->stage.p, nsplits, mn, mx, nsplits + 1,
                              w.lut));
    HIP_TRY(launch_quantize(c->stream, &c->qres, x, n, payload, w.lut, nsplits + 1));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the staged splits are reused by later calls
    return SKML_OK;
}

// Profiling hook, not in include/skml.h (like skml_debug_prof): the resident workgroups per CU of
// the quantize pass, as the runtime's occupancy query reports them for the kernel form that (xtype,
// req_bins, passed_table: non-zero for the set-splits / uniform / ZipML encodes) selects, and the
// device's CU count; their product caps the pass's grid.  Launches nothing.
int skml_debug_quantize_residency(skml_ctx* c, int32_t xtype, int32_t req_bins, int32_t passed_table,
                                  int32_t* wgs_per_cu, int32_t* cus) {
    if (!c || !wgs_per_cu || !cus || req_bins < 2) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    Workspace w;
    if (int st = ensure_ws(c, 0, &w)) return st;
    int wgs = 0;
    HIP_TRY(launch_quantize(c->stream, &c->qres, nullptr, 0, nullptr, passed_table ? w.lut : nullptr, req_bins, xtype,
                            &wgs));
    *wgs_per_cu = wgs;
    *cus = c->qres.cus;
    return SKML_OK;
}

int skml_dense_encode_f64(skml_ctx* c, const double* x, int64_t n, const skml_params* p, void* payload,
                          size_t cap) {
    skml_params def;
    p = params_or_default(p, &def, /*clear_dedup=*/false);
    int st = check_dense_args(c, x, n, p->bin_num, payload, cap);
    if (st) return st;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t chunks = n / kChunk;
    Workspace64 w;
    if ((st = ensure_ws_f64(c, chunks, &w))) return st;
    if ((st = ensure_ranks(c, n, p->bin_num))) return st;
    const uint64_t s0 = ((uint64_t)p->seed ^ kLcgMult) & kLcgMask;
    const int64_t tiles = (chunks + kLeafChunks - 1) / kLeafChunks;
    if ((st = run_sketch_f64(c, x, n, s0, w))) return st;
    Workspace wq;  // the quantize LUT lives in the fp32 workspace
    if ((st = ensure_ws(c, 0, &wq))) return st;
    {
        KernelTimer kt(c, SKML_K_SUMMARY);
        HIP_TRY(launch_summary64(c->stream, x, n, w.part, tiles, w.roots, ranks_of(c), p->bin_num,
                                 p->dedup ? 1 : 0, payload, w.raw, wq.lut));
    }
    {
        KernelTimer kt(c, SKML_K_QUANTIZE);
        HIP_TRY(launch_quantize64(c->stream, x, n, payload, wq.lut, nullptr, p->bin_num));
    }
    return SKML_OK;
}

int skml_dense_decode_f64(skml_ctx* c, const void* payload, double* out, int64_t n) {
    if (!c || !valid_payload_ptr(payload) || (n > 0 && (!out || ((uintptr_t)out) % 16)))
        return fail(SKML_E_ARG, "bad decode arguments");
    HIP_TRY(hipSetDevice(c->device));
    KernelTimer kt(c, SKML_K_DECODE);
    HIP_TRY(launch_decode64(c->stream, payload, out, n));
    return SKML_OK;
}

int skml_dense_decode_f32(skml_ctx* c, const void* payload, float* out, int64_t n) {
    if (!c || !valid_payload_ptr(payload) || (n > 0 && (!out || ((uintptr_t)out) % 16)))
        return fail(SKML_E_ARG, "bad decode arguments");
    HIP_TRY(hipSetDevice(c->device));
    KernelTimer kt(c, SKML_K_DECODE);
    HIP_TRY(launch_decode(c->stream, payload, out, n));
    return SKML_OK;
}

// A 16-bit output needs its element's alignment only (the kernels pick 16-byte or element stores).
static int dense_decode_lowp(skml_ctx* c, const void* payload, uint16_t* out, int64_t n, int otype) {
    if (!c || !valid_payload_ptr(payload) || (n > 0 && (!out || ((uintptr_t)out) % 2)))
        return fail(SKML_E_ARG, "bad decode arguments");
    HIP_TRY(hipSetDevice(c->device));
    KernelTimer kt(c, SKML_K_DECODE);
    HIP_TRY(launch_decode(c->stream, payload, out, n, otype));
    return SKML_OK;
}

int skml_dense_decode_bf16(skml_ctx* c, const void* payload, uint16_t* out, int64_t n) {
    return dense_decode_lowp(c, payload, out, n, kXBF16);
}

int skml_dense_decode_f16(skml_ctx* c, const void* payload, uint16_t* out, int64_t n) {
    return dense_decode_lowp(c, payload, out, n, kXF16);
}

}  // extern "C"

int skml::dense_sum_headers(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, int* common_bits_out,
                            int* max_bins_out) {
    if (!c || !valid_payload_ptr(payloads) || stride % 256 || P < 1 || P > 16)
        return fail(SKML_E_ARG, "bad decode_sum arguments (P in [1,16], 256-B aligned payloads)");
    HIP_TRY(hipSetDevice(c->device));
    // Gradient.sum adds gradients of one dimension (ml/gradient/Gradient.scala:44-49): every
    // payload must be a finished dense payload of exactly n codes that fits its stride.
    // the headers come back through the context's pinned staging, one copy each: a 2D copy into
    // pageable memory waits for the null stream, whatever stream it is given
    skml_dense_header* h = static_cast<skml_dense_header*>(skml::ctx_pinned(c, sizeof(skml_dense_header) * 16));
    if (!h) return fail(SKML_E_OOM, "pinned staging of the payload headers");
    for (int p = 0; p < P; p++)
        HIP_TRY(hipMemcpyAsync(h + p, static_cast<const char*>(payloads) + (size_t)p * stride, sizeof(skml_dense_header),
                               hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int p = 0; p < P; p++) {
        if (h[p].magic != SKML_DENSE_MAGIC) return fail(SKML_E_STATE, "payload %d is not a dense payload", p);
        if (h[p].status == SKML_E_NAN) return fail(SKML_E_NAN, "payload %d: Encounter NaN value", p);
        if (h[p].status != SKML_OK) return fail(SKML_E_STATE, "payload %d has status %d", p, h[p].status);
        if (h[p].n != n)
            return fail(SKML_E_ARG, "payload %d holds %lld values, the sum %lld", p, (long long)h[p].n, (long long)n);
        if (h[p].bin_num < 2 || h[p].bin_num > SKML_MAX_BINS || h[p].code_bits != code_bits_for(h[p].bin_num) ||
            h[p].bin_num > h[p].req_bins || h[p].codes_offset != (int64_t)dense_codes_offset(h[p].req_bins) ||
            skml_dense_payload_bytes(n, h[p].req_bins) > stride)
            return fail(SKML_E_ARG, "payload %d: inconsistent header or larger than the stride %zu", p, stride);
    }
    int common_bits = h[0].code_bits, max_bins = h[0].bin_num;
    for (int p = 1; p < P; p++) {
        if (h[p].code_bits != common_bits) common_bits = 0;
        max_bins = std::max(max_bins, (int)h[p].bin_num);
    }
    *common_bits_out = common_bits;
    *max_bins_out = max_bins;
    return SKML_OK;
}

extern "C" {

static int dense_decode_sum_x(skml_ctx* c, const void* payloads, int32_t P, size_t stride, void* out, int otype,
                              int64_t n, double scale) {
    if (c && n > 0 && (!out || ((uintptr_t)out) % (otype == kXF32 ? 16 : 2)))
        return fail(SKML_E_ARG, "bad decode_sum arguments (P in [1,16], 256-B aligned payloads)");
    int common_bits = 0, max_bins = 0;
    if (const int st = dense_sum_headers(c, payloads, P, stride, n, &common_bits, &max_bins)) return st;
    KernelTimer kt(c, SKML_K_DECODE_SUM);
    HIP_TRY(launch_decode_sum(c->stream, payloads, P, stride, out, n, scale, common_bits, max_bins, otype));
    return SKML_OK;
}

int skml_dense_decode_sum_f32(skml_ctx* c, const void* payloads, int32_t P, size_t stride, float* out,
                              int64_t n, double scale) {
    return dense_decode_sum_x(c, payloads, P, stride, out, kXF32, n, scale);
}

int skml_dense_decode_sum_bf16(skml_ctx* c, const void* payloads, int32_t P, size_t stride, uint16_t* out,
                               int64_t n, double scale) {
    return dense_decode_sum_x(c, payloads, P, stride, out, kXBF16, n, scale);
}

int skml_dense_decode_sum_f16(skml_ctx* c, const void* payloads, int32_t P, size_t stride, uint16_t* out,
                              int64_t n, double scale) {
    return dense_decode_sum_x(c, payloads, P, stride, out, kXF16, n, scale);
}

int skml_dense_bins_i32(skml_ctx* c, const void* payload, int32_t* bins, int64_t n) {
    if (!c || !valid_payload_ptr(payload) || (n > 0 && !bins)) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_bins(c->stream, payload, bins, n));
    return SKML_OK;
}

int skml_dense_info(skml_ctx* c, const void* payload, skml_dense_header* hdr, double* splits,
                    int32_t splits_cap) {
    if (!c || !valid_payload_ptr(payload) || !hdr) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(hdr, payload, sizeof(*hdr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (hdr->magic != SKML_DENSE_MAGIC) return fail(SKML_E_STATE, "not a dense payload");
    if (splits && hdr->status == SKML_OK) {
        const int ns = hdr->bin_num - 1;
        if (ns > splits_cap) return fail(SKML_E_ARG, "splits capacity %d < %d", splits_cap, ns);
        HIP_TRY(hipMemcpyAsync(splits, (const char*)payload + kHeaderBytes, sizeof(double) * ns,
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (hdr->status == SKML_E_NAN) return fail(SKML_E_NAN, "Encounter NaN value");
    return hdr->status;
}

int skml_dense_times_by(skml_ctx* c, void* payload, double x) {
    if (!c || !valid_payload_ptr(payload)) return fail(SKML_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_times_by(c->stream, payload, x));
    return SKML_OK;
}

}  // extern "C"
