// skml_sparse_payload.cpp -- the library-owned sparse payload (include/skml.h, "Sparse path"): the
// pool of its device blocks, its release, the small services the sparse host files share, the
// accessors and the debug hooks.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "skml_sparse_host.hpp"

using namespace skml;

namespace {

// Device blocks of encoded payloads, recycled across encodes: a hipMalloc / hipFree pair per
// payload cost more than all the rest of an encode's host work (hipFree also waits for the
// device).  Every sparse call completes its device work before it returns (a failing encode
// synchronises before releasing), so a freed payload's block has no pending users.
struct BlockPool {
    struct Blk {
        int dev;
        void* p;
        size_t cap;
    };
    std::mutex mu;
    std::vector<Blk> free;
};
constexpr size_t kPoolMaxBlocks = 8;
BlockPool& block_pool() {
    static BlockPool* bp = new BlockPool();  // never destroyed: payloads may be freed during exit
    return *bp;
}
void pool_drop(std::vector<BlockPool::Blk>& v, int cur_dev) {
    for (const auto& b : v) {
        (void)hipSetDevice(b.dev);
        (void)hipFree(b.p);
    }
    if (!v.empty()) (void)hipSetDevice(cur_dev);
}

}  // namespace

namespace skml {

thread_local int t_merge_path = 0;
// skml_debug_sparse_scratch_fail: simulate failed MinMax staging allocations (tests only)
std::atomic<int> g_fail_cellbuf{0};
// skml_debug_sparse_sum_budget: Gradient.sum's scratch budget per batch (tests only; 0: kSumBudget)
std::atomic<int64_t> g_sum_budget{0};
thread_local int32_t t_sum_batches = 0, t_sum_launches = 0;

// smallest pooled block of `dev` holding `bytes` without wasting more than bytes + 64 MiB
void* block_get(int dev, size_t bytes, size_t* cap) {
    BlockPool& bp = block_pool();
    {
        std::lock_guard<std::mutex> lk(bp.mu);
        size_t best = bp.free.size();
        for (size_t i = 0; i < bp.free.size(); i++) {
            const BlockPool::Blk& b = bp.free[i];
            if (b.dev == dev && b.cap >= bytes && b.cap <= 2 * bytes + ((size_t)64 << 20) &&
                (best == bp.free.size() || b.cap < bp.free[best].cap))
                best = i;
        }
        if (best < bp.free.size()) {
            void* p = bp.free[best].p;
            *cap = bp.free[best].cap;
            bp.free.erase(bp.free.begin() + (ptrdiff_t)best);
            return p;
        }
    }
    const size_t c = align_up(std::max<size_t>(bytes, 1), (size_t)2 << 20);
    void* p = nullptr;
    if (hipMalloc(&p, c) != hipSuccess) {  // out of memory: return this device's pooled blocks, retry once
        (void)hipGetLastError();
        std::vector<BlockPool::Blk> drop;
        {
            std::lock_guard<std::mutex> lk(bp.mu);
            for (size_t i = 0; i < bp.free.size();)
                if (bp.free[i].dev == dev) {
                    drop.push_back(bp.free[i]);
                    bp.free.erase(bp.free.begin() + (ptrdiff_t)i);
                } else {
                    i++;
                }
        }
        pool_drop(drop, dev);
        if (hipMalloc(&p, c) != hipSuccess) return nullptr;
    }
    *cap = c;
    return p;
}
void block_put(int dev, void* p, size_t cap) {
    BlockPool& bp = block_pool();
    std::vector<BlockPool::Blk> drop;
    {
        std::lock_guard<std::mutex> lk(bp.mu);
        bp.free.push_back(BlockPool::Blk{dev, p, cap});
        while (bp.free.size() > kPoolMaxBlocks) {
            drop.push_back(bp.free.front());
            bp.free.erase(bp.free.begin());
        }
    }
    pool_drop(drop, dev);
}

void sparse_release(skml_sparse* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->block) {
        block_put(s->device, s->block, s->block_cap);
    } else {
        if (s->qpayload) (void)hipFree(s->qpayload);
        if (s->g_dev) (void)hipFree(s->g_dev);
        if (s->tables) (void)hipFree(s->tables);
        if (s->flag_words) (void)hipFree(s->flag_words);
        if (s->delta_words) (void)hipFree(s->delta_words);
    }
    if (s->huff_words) (void)hipFree(s->huff_words);
    if (s->wire_dev) (void)hipFree(s->wire_dev);
    delete s;
}

int upload_groups(skml_ctx* c, skml_sparse* s) {
    for (int g = 0; g < kMaxGroups; g++) s->g.inv_cols[g] = s->g.cols[g] > 0 ? 1.0 / (double)s->g.cols[g] : 0.0;
    HIP_TRY(hipMemcpyAsync(s->g_dev, &s->g, sizeof(SpGroups), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SKML_OK;
}

int sync_to_host(skml_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!bytes) return SKML_OK;
    void* pin = ctx_pinned(c, bytes);
    if (!pin) return fail(SKML_E_OOM, "pinned staging of %zu bytes", bytes);
    HIP_TRY(hipMemcpyAsync(pin, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(dst, pin, bytes);
    return SKML_OK;
}

int scan_tiles(skml_ctx* c, uint64_t* sums, int64_t tiles, int K, uint64_t* totals) {
    HIP_TRY(launch_scan_cols(c->stream, sums, tiles, K));
    if (totals) return sync_to_host(c, totals, sums + tiles * K, sizeof(uint64_t) * (size_t)K);
    return SKML_OK;
}

}  // namespace skml

// Copy bits [b0, b0 + nbits) of a device word stream into host words starting at bit 0.
static int extract_bits(skml_ctx* c, const uint64_t* words, int64_t b0, int64_t nbits, uint64_t* out) {
    const int64_t nw = (nbits + 63) / 64;
    if (nw == 0) return SKML_OK;
    const int64_t w0 = b0 >> 6, w1 = (b0 + nbits - 1) >> 6;
    std::vector<uint64_t> buf((size_t)(w1 - w0 + 2), 0);
    if (int e = sync_to_host(c, buf.data(), words + w0, sizeof(uint64_t) * (size_t)(w1 - w0 + 1))) return e;
    const int sh = (int)(b0 & 63);
    for (int64_t i = 0; i < nw; i++) {
        uint64_t v = buf[(size_t)i] >> sh;
        if (sh) v |= buf[(size_t)i + 1] << (64 - sh);
        out[i] = v;
    }
    const int tail = (int)(nbits & 63);
    if (tail) out[nw - 1] &= (1ULL << tail) - 1ULL;
    return SKML_OK;
}

extern "C" {

int skml_sparse_times_by(skml_sparse* s, double x) {
    if (!s) return fail(SKML_E_ARG, "NULL argument");
    for (double& v : s->qvalues) v *= x;  // SparseVectorCompressor.timesBy (:128-134)
    s->qv_dev_ok = false;  // the device copy is re-uploaded by the next restore
    return SKML_OK;
}

int skml_sparse_values(const skml_sparse* s, double* out, int32_t cap) {
    if (!s || !out) return fail(SKML_E_ARG, "NULL argument");
    const size_t k = std::min<size_t>(s->qvalues.size(), (size_t)std::max(cap, 0));
    std::memcpy(out, s->qvalues.data(), sizeof(double) * k);
    return SKML_OK;
}

int skml_sparse_nnz(const skml_sparse* s, int64_t* nnz) {
    if (!s || !nnz) return fail(SKML_E_ARG, "NULL argument");
    *nnz = s->nnz;
    return SKML_OK;
}

int skml_sparse_quant_info(const skml_sparse* s, skml_dense_header* hdr, double* splits_host, int32_t cap) {
    if (!s || !hdr) return fail(SKML_E_ARG, "NULL argument");
    *hdr = s->hdr;
    if (splits_host) {
        const size_t k = std::min<size_t>(s->splits.size(), (size_t)std::max(cap, 0));
        std::memcpy(splits_host, s->splits.data(), sizeof(double) * k);
    }
    return SKML_OK;
}

int skml_sparse_group_info(skml_ctx* c, const skml_sparse* s, int32_t g, skml_sparse_group* info,
                           int32_t* table_host, uint64_t* flag_words_host, uint64_t* delta_words_host) {
    if (!c || !s || !info || g < 0 || g >= s->g.G) return fail(SKML_E_ARG, "bad group query");
    HIP_TRY(hipSetDevice(c->device));
    const SpGroups& G = s->g;
    std::memset(info, 0, sizeof(*info));
    info->size = (int32_t)(G.gstart[g + 1] - G.gstart[g]);
    if (info->size == 0) return SKML_OK;  // null sketch / encoder (GroupedMinMaxSketch.java:105-109)
    info->col_num = G.cols[g];
    for (int r = 0; r < G.rows; r++) info->hash_ids[r] = G.hash_ids[g][r];
    info->num_intervals = G.m[g];
    info->flag_kind = G.kind[g];
    info->n_flag_bits = G.fb[g + 1] - G.fb[g];
    info->n_delta_bits = G.db[g + 1] - G.db[g];
    if (table_host)
        if (int e = sync_to_host(c, table_host, s->tables + G.tab_off[g], sizeof(int32_t) * (size_t)G.rows * G.cols[g]))
            return e;
    if (flag_words_host)
        if (int e = extract_bits(c, s->flag_words, G.fb[g], info->n_flag_bits, flag_words_host)) return e;
    if (delta_words_host)
        if (int e = extract_bits(c, s->delta_words, G.db[g], info->n_delta_bits, delta_words_host)) return e;
    return SKML_OK;
}

int skml_debug_sparse_merge_path(void) { return t_merge_path; }

int skml_debug_sparse_scratch_fail(int on) {
    g_fail_cellbuf.store(on ? 1 : 0);
    return SKML_OK;
}

int64_t skml_debug_sparse_sum_budget(int64_t bytes) { return g_sum_budget.exchange(bytes > 0 ? bytes : 0); }

int skml_debug_sparse_sum_path(int32_t* batches, int32_t* launches) {
    if (!batches || !launches) return fail(SKML_E_ARG, "NULL argument");
    *batches = t_sum_batches;
    *launches = t_sum_launches;
    return SKML_OK;
}

int skml_sparse_free(skml_sparse* s) {
    sparse_release(s);
    return SKML_OK;
}

}  // extern "C"
