// skml_sparse_minmax.hip -- CDNA4 (gfx950) kernels of the sparse codec: group prep with the MinMaxSketch
// insert, and the restore.
//   k_group_prep     DeltaAdaptiveEncoder.encode step 1 (binary/DeltaAdaptiveEncoder.java:54-71)
//                    and MinMaxSketch.insert (frequency/MinMaxSketch.java:48-55) as a 64-bit
//                    atomicMin on (|bin-zero|, key, bin): the smaller distance wins, ties keep the
//                    earlier (= smaller key, keys ascend within a group) insert.
//   k_unary_* / k_dec_*  DeltaAdaptiveEncoder.decode (:114-146) in parallel: unary flags are
//                    resolved by selecting zero bits, delta offsets and keys by scans.
// The insert and the restore share this translation unit.  The optimiser propagates a helper's
// argument ranges from all the callers it sees: without the restore's calls of delta_shape, __clz is
// only ever given a non-zero argument (divu32_make) and k_group_prep compiles to other code.
#include <algorithm>

#include "skml_device.hpp"
#include "skml_sparse.h"
#include "skml_sparse_device.hpp"

namespace skml {

// ---------------------------------------------------------------------------------------------
// Java Int2IntHash family (hash/BJHash.java:10-20, Mix64Hash.java:10-21, TWHash.java:10-20,
// BKDRHash.java:13-21), int32 wrap-around arithmetic; code % size folded non-negative.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sar(uint32_t c, int s) { return (uint32_t)((int32_t)c >> s); }

// BKDRHash's digit loop over a non-negative key, three decimal digits per step: a full chunk r
// (digits d0 d1 d2, d0 the lowest) advances the code to code * s^3 + (d0 s + d1) s + d2, the last
// chunk by as many digits as it has.  Every product but code * s^k has both operands below 2^24
// (r < 1000, d < 10, s <= 13131, k / 1000 < 2^23, (d0 s + d1) s < 2^31), so it is a full-rate
// 24-bit multiply instead of a quarter-rate 32-bit one; k / 1000 as the truncated double product
// with RN(1/1000), which lies above 1/1000: never below the quotient, and below the next integer
// by more than the product's rounding for every 32-bit k.  Checked exhaustively against the digit
// loop on the host (tests/test_hash_arith.py).
__device__ __forceinline__ uint32_t div1000(uint32_t k) { return (uint32_t)((double)k * 0.001); }
__device__ __forceinline__ uint32_t bkdr3(uint32_t seed, uint32_t r) {  // r < 1000: d0 s^2 + d1 s + d2
    const uint32_t t = __umul24(r, 205u) >> 11, h = __umul24(r, 41u) >> 12;  // r / 10, r / 100
    return __umul24(__umul24(r - 10u * t, seed) + (t - 10u * h), seed) + h;
}
__device__ __forceinline__ uint32_t bkdr_chunks(uint32_t seed, uint32_t k) {
    const uint32_t s2 = seed * seed, s3 = s2 * seed;
    uint32_t c = 0;
    while (k >= 1000u) {
        const uint32_t q = div1000(k);
        c = c * s3 + bkdr3(seed, k - __umul24(q, 1000u));
        k = q;
    }
    if (k >= 100u) {
        c = c * s3 + bkdr3(seed, k);
    } else if (k >= 10u) {
        const uint32_t t = __umul24(k, 205u) >> 11;
        c = c * s2 + __umul24(k - 10u * t, seed) + t;
    } else if (k) {
        c = c * seed + k;
    }
    return c;
}

__device__ __forceinline__ uint32_t java_hash_mix(int id, int32_t key) {
    uint32_t c = (uint32_t)key;
    if (id == 0) {
        c = (c + 0x7ed55d16u) + (c << 12);
        c = (c ^ 0xc761c23cu) ^ sar(c, 19);
        c = (c + 0x165667b1u) + (c << 5);
        c = (c + 0xd3a2646cu) ^ (c << 9);
        c = (c + 0xfd7046c5u) + (c << 3);
        c = (c ^ 0xb55a4f09u) ^ sar(c, 16);
    } else if (id == 1) {
        c = ~c + (c << 21);
        c = c ^ sar(c, 24);
        c = (c + (c << 3)) + (c << 8);
        c = c ^ sar(c, 14);
        c = (c + (c << 2)) + (c << 4);
        c = c ^ sar(c, 28);
        c = c + (c << 31);
    } else if (id == 2) {
        c = ~c + (c << 15);
        c = c ^ sar(c, 12);
        c = c + (c << 2);
        c = c ^ sar(c, 4);
        c = c * 2057u;
        c = c ^ sar(c, 16);
    } else {
        const uint32_t seed = id == 3 ? 31u : id == 4 ? 131u : id == 5 ? 267u : id == 6 ? 1313u : 13131u;
        c = 0;
        if (key >= 0) {  // every valid key: Java's int % and / are the unsigned ones
            c = bkdr_chunks(seed, (uint32_t)key);
        } else {
            int32_t k = key;
            while (k != 0) {
                c = seed * c + (uint32_t)(k % 10);
                k /= 10;
            }
        }
    }
    return c;
}
__device__ __forceinline__ int32_t java_hash(int id, int32_t key, int32_t size) {
    const int32_t r = (int32_t)java_hash_mix(id, key) % size;
    return r >= 0 ? r : r + size;
}
// The same with `% size` folded non-negative as r - floor(r * (1/size)) * size: the double
// product is within one of the true quotient and one correction step makes the result exact (an
// integer division by a run-time divisor is a long instruction sequence on the GPU).
// For size <= 2^30, in 32 bits: the quotient is off by at most one, so the uncorrected remainder
// lies in [-size, 2 size) (tests/test_hash_arith.py).
__device__ __forceinline__ int32_t java_hash_fm32(int id, int32_t key, int32_t size, double inv) {
    const int32_t r = (int32_t)java_hash_mix(id, key);
    const int32_t q = (int32_t)floor((double)r * inv);
    int32_t m = (int32_t)((uint32_t)r - (uint32_t)q * (uint32_t)size);
    if (m < 0) m += size;
    else if (m >= size) m -= size;
    return m;
}
__device__ __forceinline__ int32_t java_hash_fm(int id, int32_t key, int32_t size, double inv) {
    if (size <= 0x40000000) return java_hash_fm32(id, key, size, inv);
    const int32_t r = (int32_t)java_hash_mix(id, key);
    const int64_t q = (int64_t)floor((double)r * inv);
    int64_t m = (int64_t)r - q * (int64_t)size;
    if (m < 0) m += size;
    else if (m >= size) m -= size;
    return (int32_t)m;
}

// 4 elements' cells of one MinMax row with the hash fixed at compile time, as 32-bit offsets
// (row0: the row's first cell, relative): for a k_dec_keys tile inside one group, whose lanes all
// use the same hash id, java_hash_mix folds to the one hash instead of computing every variant.
// SKML_DEC_INTMOD (A/B builds): 1 = the modulus by a 32-bit magic-number division (java_mod, as the
// encode's MinMax insert does) instead of the double-precision quotient.
#ifndef SKML_DEC_INTMOD
#define SKML_DEC_INTMOD 0
#endif
template <int ID, typename DV>
__device__ __forceinline__ void dec_row_cells(const int32_t (&key)[4], int64_t i0, int64_t n, int64_t row0,
                                              int32_t cols, double inv, const DV& dv, uint32_t (&rel)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
#ifdef SKML_ABLATE_DEC_HASH  // timing ablation only (wrong cells): the hashes priced
        rel[j] = (uint32_t)(row0 + ((uint32_t)key[j] & 0xFFFFu));
        continue;
#endif
        // every element is hashed, those past n too (their keys are whatever the prefix left and
        // their cells lie inside the row; nothing of theirs is stored): no exec-mask branches
        // around the digit loops and the gathers
        (void)i0, (void)n;
        if constexpr (SKML_DEC_INTMOD)
            rel[j] = (uint32_t)(row0 + dv(java_hash_mix(ID, key[j])));
        else
            rel[j] = (uint32_t)(row0 + java_hash_fm32(ID, key[j], cols, inv));
    }
}

// =============================================================================================
// Group prep: deltas / bitsNeeded / order check / MinMax insert
// =============================================================================================
// MinMaxSketch.insert, bucketed: every (element, row) pair targets table cell c; pairs are
// counted per bucket of kMmBucketCells cells, scattered into bucket order, and each bucket's minimum is
// taken with LDS atomics by one workgroup (random global 64-bit atomics were HBM-latency bound).
// Pair word: |bin - zero| [63:48], key [47:17], bin < zero [16], cell % kMmBucketCells [14:0]; its
// value with the cell bits cleared orders by (distance, key): the smaller distance wins and ties
// keep the earlier insert (keys ascend within a group).
constexpr int kMmBucketBits = SKML_MM_BUCKET_BITS;
static_assert(kMmBucketBits >= 13 && kMmBucketBits <= 15, "pair layouts hold 13..15 cell bits");
constexpr int kMmSubBits = 13;  // key-carrying pairs: u64 LDS minima over 8192-cell sub-ranges
constexpr int kMmSubCells = 1 << kMmSubBits;
constexpr int kMmBucketCells = kMmCellsPerBucket;
static_assert(kMmBucketCells == 1 << kMmBucketBits, "bucket size");
constexpr int kMmLdsBuckets = 8192;  // per-workgroup bucket tables in LDS up to this many (96 KB in the scatter)
constexpr int kMmThreads = 1024;  // count / scatter workgroups: big tiles, long per-bucket runs
#ifndef SKML_MM_BATCH
#define SKML_MM_BATCH 4
#endif
constexpr int kMmBatch = SKML_MM_BATCH;  // elements per thread in flight (count, scatter)
#ifndef SKML_BUCKET_BATCH
#define SKML_BUCKET_BATCH 8
#endif
constexpr int kBucketBatch = SKML_BUCKET_BATCH;  // pairs per thread in flight in the bucket minima

// a group's MinMaxSketch shape, staged in LDS by the count pass
// Unsigned division by a run-time d through a multiplier (the round-up method: exact for every
// 32-bit dividend); sh < 0 marks d == 1.
struct DivU32 {
    uint32_t m;
    int32_t sh;
};
__device__ __forceinline__ DivU32 divu32_make(uint32_t d) {
    if (d <= 1) return DivU32{0u, -1};
    const int l = 32 - __clz(d - 1);  // ceil(log2 d)
    return DivU32{(uint32_t)(((((uint64_t)1 << l) - d) << 32) / d + 1), l - 1};
}
__device__ __forceinline__ uint32_t divu32(uint32_t n, DivU32 v) {
    const uint32_t t = __umulhi(n, v.m);
    return (t + ((n - t) >> 1)) >> v.sh;
}
// Int2IntHash's `code %= size; return code >= 0 ? code : code + size` (the floor modulus)
__device__ __forceinline__ int32_t java_mod(int32_t code, int32_t d, DivU32 v) {
    if (v.sh < 0) return 0;
    const uint32_t u = code < 0 ? 0u - (uint32_t)code : (uint32_t)code;
    const uint32_t rem = u - divu32(u, v) * (uint32_t)d;
    return (code < 0 && rem) ? d - (int32_t)rem : (int32_t)rem;
}

// a group's MinMaxSketch shape, staged in LDS by the count pass
struct MmGroup {
    int64_t tab_off;
    double inv;
    int32_t cols;
    DivU32 div;
    int32_t hid[kMaxRows];
};
__device__ __forceinline__ void load_mm_groups(const SpGroups* gp, MmGroup* GP) {
    for (int g = threadIdx.x; g < gp->G; g += blockDim.x) {
        GP[g].tab_off = gp->tab_off[g];
        GP[g].inv = gp->inv_cols[g];
        GP[g].cols = gp->cols[g];
        GP[g].div = divu32_make((uint32_t)gp->cols[g]);
        for (int r = 0; r < kMaxRows; r++) GP[g].hid[r] = gp->hash_ids[g][r];
    }
}
// reserved pair slots of a (tile, bucket) range: whole 128-byte lines (16 wide or 32 narrow
// pairs), padding = kMmNoPair / kMmNoPair32
__device__ __forceinline__ uint32_t mm_pad(uint32_t c) { return (c + 15u) & ~15u; }
__device__ __forceinline__ uint32_t mm_pad(uint32_t c, bool narrow) {
    return narrow ? (c + 31u) & ~31u : (c + 15u) & ~15u;
}
constexpr uint64_t kMmNoPair = ~0ull;
constexpr uint32_t kMmNoPair32 = ~0u;
// Narrow pair word (SpGroups.mm_narrow): |bin - zero| [31:B+1], bin < zero [B], cell % 2^B
// [B-1:0] with B = kMmBucketBits (|bin - zero| < 65536 fits 31 - B >= 16 bits).  In a one-sided
// group the sign bit is constant, so the minimum over a cell is the nearest bin.
__device__ __forceinline__ uint32_t mm_pair32(int32_t bin, int32_t zero, int64_t cell) {
    return ((uint32_t)mm_dist(bin, zero) << (kMmBucketBits + 1)) | ((bin < zero ? 1u : 0u) << kMmBucketBits) |
           (uint32_t)(cell & (kMmBucketCells - 1));
}
__device__ __forceinline__ int64_t mm_cell(const SpGroups* gp, int g, int r, int32_t key) {
    const int32_t cols = gp->cols[g];
    return gp->tab_off[g] + (int64_t)r * cols + java_hash_fm(gp->hash_ids[g][r], key, cols, gp->inv_cols[g]);
}
__device__ __forceinline__ uint64_t mm_pair(int32_t key, int32_t bin, int32_t zero, int64_t cell) {
    return ((uint64_t)mm_dist(bin, zero) << 48) | ((uint64_t)(uint32_t)key << 17) |
           ((uint64_t)(bin < zero ? 1u : 0u) << 16) | (uint64_t)(cell & (kMmBucketCells - 1));
}

// BKDRHash over 3-digit chunks (hash/BKDRHash.java:13-21).  The loop consumes a key's decimal
// digits least significant first, code = code * seed + digit, so a full 3-digit chunk c (digits
// d0 d1 d2, d0 the lowest) advances the code to code * seed^3 + (d0 seed^2 + d1 seed + d2), and
// the last chunk v (1..3 digits) to code * seed^len(v) + BKDR(v).  LDS tables per seed:
// f3[c] for full chunks, b3[v] = BKDR(v); one quarter-rate multiply per chunk instead of two per
// digit.  Keys are >= 0 here (a negative key fails the order check; java_hash_mix keeps the
// reference's signed digits for it).
constexpr int kBkSeeds = 5;  // hash ids 3..7
struct BkdrTables {
    uint32_t f3[kBkSeeds][1000];
    uint32_t b3[kBkSeeds][1000];
};
__device__ __forceinline__ uint32_t bkdr_seed(int id) {
    return id == 3 ? 31u : id == 4 ? 131u : id == 5 ? 267u : id == 6 ? 1313u : 13131u;
}
__device__ __forceinline__ void load_bkdr_tables(BkdrTables* T) {
    for (int e = threadIdx.x; e < kBkSeeds * 1000; e += blockDim.x) {
        const int si = e / 1000, v = e % 1000;
        const uint32_t sd = bkdr_seed(si + 3);
        const uint32_t d0 = (uint32_t)v % 10u, d1 = (uint32_t)v / 10u % 10u, d2 = (uint32_t)v / 100u;
        T->f3[si][v] = (d0 * sd + d1) * sd + d2;
        uint32_t c = 0, k = (uint32_t)v;
        while (k) {
            c = c * sd + k % 10u;
            k /= 10u;
        }
        T->b3[si][v] = c;
    }
}
template <int ID>
__device__ __forceinline__ uint32_t bkdr_fast(uint32_t k, const BkdrTables* T) {
    constexpr uint32_t sd = ID == 3 ? 31u : ID == 4 ? 131u : ID == 5 ? 267u : ID == 6 ? 1313u : 13131u;
    constexpr uint32_t s2 = sd * sd, s3 = s2 * sd;
    uint32_t c = 0;
    while (k >= 1000u) {
        const uint32_t q = k / 1000u;
        c = c * s3 + T->f3[ID - 3][k - q * 1000u];
        k = q;
    }
    const uint32_t pw = k >= 100u ? s3 : k >= 10u ? s2 : sd;
    return k ? c * pw + T->b3[ID - 3][k] : c;
}

// One row's cells of a batch whose group (and so hash) is uniform: the hash specialised at
// compile time, the modulus by multiplication.  Same cells as java_hash_fm.
template <int ID>
__device__ __forceinline__ void mm_cells(const int32_t (&key)[kMmBatch], int64_t base, int64_t c1, int64_t n, int r,
                                         int64_t row0, const MmGroup& q, const BkdrTables* BK,
                                         int32_t* __restrict__ cells_out, bool lds_b, uint32_t* BH,
                                         unsigned long long* __restrict__ bucket_count) {
    const int32_t cols = q.cols;
    const DivU32 dv = q.div;
#pragma unroll
    for (int u = 0; u < kMmBatch; u++) {
        const int64_t i = base + u * kMmThreads + threadIdx.x;
        if (i >= c1) continue;
        uint32_t h;
#ifdef SKML_ABLATE_GP_HASH  // timing ablation only (wrong cells): the insert's hashes priced
        h = (uint32_t)key[u] * 2654435761u;
#else
        if constexpr (ID >= 3) h = key[u] >= 0 ? bkdr_fast<ID>((uint32_t)key[u], BK) : java_hash_mix(ID, key[u]);
        else h = java_hash_mix(ID, key[u]);
#endif
        const int64_t cell = row0 + java_mod((int32_t)h, cols, dv);
        if (cells_out) cells_out[(int64_t)r * n + i] = (int32_t)cell;  // hashed once, reused by the scatter
        const int b = (int)(cell >> kMmBucketBits);
        if (lds_b) atomicAdd(&BH[b], 1u);
        else atomicAdd(&bucket_count[b], 1ull);
    }
}

// Deltas, bitsNeeded histogram and order check (DeltaAdaptiveEncoder.encode step 1) plus the
// per-bucket pair counts of the MinMax insert.
// 8 waves per SIMD (64 VGPRs, with kMmBatch = 4): two 1,024-thread workgroups per CU instead of
// one at 103 VGPRs and 8 elements in flight (C3: 195 -> 176 us; at 8 elements the cap spills)
#ifndef SKML_GP_WAVES
#define SKML_GP_WAVES 8
#endif
__global__ __launch_bounds__(kMmThreads, SKML_GP_WAVES) void k_group_prep(const int32_t* __restrict__ gkeys, int64_t n,
                                                           const SpGroups* __restrict__ gp,
                                                           uint8_t* __restrict__ need, uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ err,
                                                           unsigned long long* __restrict__ bucket_count,
                                                           int nbuckets, int32_t* __restrict__ cells_out,
                                                           uint32_t* __restrict__ tile_off, int64_t chunk) {
    if (gp->status) return;
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ uint32_t H[kMaxGroups * kDeltaHist];
    __shared__ MmGroup GP[kMaxGroups];
    __shared__ BkdrTables BKs;
    extern __shared__ uint32_t BH[];  // nbuckets counters (dynamic: occupancy follows the table size)
    // need == nullptr: the MinMax part only; bucket_count == nullptr: the DeltaAdaptive part only
    const bool do_delta = need != nullptr, do_mm = bucket_count != nullptr;
    const int G = gp->G, rows = do_mm ? gp->rows : 0;
    const bool lds_b = nbuckets <= kMmLdsBuckets;
    const BkdrTables* BK = &BKs;
    load_starts(gp, S);
    load_mm_groups(gp, GP);
    if (rows > 0) load_bkdr_tables(&BKs);
    for (int j = threadIdx.x; j < G * kDeltaHist; j += kMmThreads) H[j] = 0;
    if (lds_b)
        for (int j = threadIdx.x; j < nbuckets; j += kMmThreads) BH[j] = 0;
    __syncthreads();
    uint32_t bad = 0;
    const int64_t c0 = (int64_t)blockIdx.x * chunk, c1 = std::min<int64_t>(n, c0 + chunk);
    // kMmBatch elements per thread in flight: their keys and predecessors load together
    for (int64_t base = c0; base < c1; base += kMmBatch * kMmThreads) {
        int32_t key[kMmBatch], prv[kMmBatch];
#pragma unroll
        for (int u = 0; u < kMmBatch; u++) {
            const int64_t i = base + u * kMmThreads + threadIdx.x;
            const int64_t j = i < c1 ? i : c1 - 1;
            key[u] = gkeys[j];
            prv[u] = do_delta && j > 0 ? gkeys[j - 1] : 0;
        }
        // almost every batch lies inside one group: then its hash ids are workgroup-uniform and
        // each row's cells come from a loop specialised for that hash
        const int64_t last = std::min<int64_t>(c1, base + kMmBatch * kMmThreads) - 1;
        const int g_lo = group_of_elem(S, base), g_hi = group_of_elem(S, last);
        const bool one = g_lo == g_hi;
        int gg[kMmBatch];
#pragma unroll
        for (int u = 0; u < kMmBatch; u++) {
            const int64_t i = base + u * kMmThreads + threadIdx.x;
            gg[u] = 0;
            if (i >= c1) continue;
            const int g = one ? g_lo : group_of_elem(S, i);
            gg[u] = g;
            if (!do_delta) continue;
            const bool first = i == S[g];
            const int32_t d = first ? key[u] : (int32_t)((uint32_t)key[u] - (uint32_t)prv[u]);
            int nb;
            if (first && d == 0) nb = 1;
            else {
                if (d <= 0) bad = 1;  // Maths.log2nlz: "Log for <d>" (util/Maths.java:16-21)
                nb = d > 0 ? 32 - __clz(d) : 1;
            }
            need[i] = (uint8_t)nb;
#ifndef SKML_ABLATE_GP_HIST  // timing ablation only (wrong histogram)
            atomicAdd(&H[g * kDeltaHist + nb], 1u);
#endif
        }
        if (one) {
            const MmGroup& q = GP[g_lo];
            for (int r = 0; r < rows; r++) {
                const int id = __builtin_amdgcn_readfirstlane(q.hid[r]);
                const int64_t row0 = q.tab_off + (int64_t)r * q.cols;
                switch (id) {
                    case 0: mm_cells<0>(key, base, c1, n, r, row0, q, BK, cells_out, lds_b, BH, bucket_count); break;
                    case 1: mm_cells<1>(key, base, c1, n, r, row0, q, BK, cells_out, lds_b, BH, bucket_count); break;
                    case 2: mm_cells<2>(key, base, c1, n, r, row0, q, BK, cells_out, lds_b, BH, bucket_count); break;
                    case 3: mm_cells<3>(key, base, c1, n, r, row0, q, BK, cells_out, lds_b, BH, bucket_count); break;
                    case 4: mm_cells<4>(key, base, c1, n, r, row0, q, BK, cells_out, lds_b, BH, bucket_count); break;
                    case 5: mm_cells<5>(key, base, c1, n, r, row0, q, BK, cells_out, lds_b, BH, bucket_count); break;
                    case 6: mm_cells<6>(key, base, c1, n, r, row0, q, BK, cells_out, lds_b, BH, bucket_count); break;
                    default: mm_cells<7>(key, base, c1, n, r, row0, q, BK, cells_out, lds_b, BH, bucket_count); break;
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < kMmBatch; u++) {
                const int64_t i = base + u * kMmThreads + threadIdx.x;
                if (i >= c1) continue;
                const MmGroup& q = GP[gg[u]];
                for (int r = 0; r < rows; r++) {
                    const int64_t cell =
                        q.tab_off + (int64_t)r * q.cols + java_hash_fm(q.hid[r], key[u], q.cols, q.inv);
                    if (cells_out) cells_out[(int64_t)r * n + i] = (int32_t)cell;
                    const int b = (int)(cell >> kMmBucketBits);
                    if (lds_b) atomicAdd(&BH[b], 1u);
                    else atomicAdd(&bucket_count[b], 1ull);
                }
            }
        }
    }
    if (bad) atomicOr(err, 1u);
    __syncthreads();
    if (do_delta)
        for (int j = threadIdx.x; j < G * kDeltaHist; j += kMmThreads)
            if (H[j]) atomicAdd(&hist[j], H[j]);
    if (lds_b && rows > 0) {
        if (tile_off) {  // reserve this tile's range in every bucket: 8 independent atomics in flight
            const bool narrow = gp->mm_narrow != 0;
            // Ranges are padded to whole 128-byte lines, so every line of the pair array is written by
            // one workgroup only (no partial-line write-backs from two XCDs' L2s).
            uint32_t* row = tile_off + (int64_t)blockIdx.x * nbuckets;
            for (int j0 = threadIdx.x; j0 < nbuckets; j0 += 8 * kMmThreads) {
                unsigned long long o[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int j = j0 + u * kMmThreads;
                    o[u] = (j < nbuckets && BH[j]) ? atomicAdd(&bucket_count[j], (unsigned long long)mm_pad(BH[j], narrow))
                                                   : 0ull;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int j = j0 + u * kMmThreads;
                    if (j < nbuckets) row[j] = (uint32_t)o[u];
                }
            }
        } else {
            for (int j = threadIdx.x; j < nbuckets; j += kMmThreads)
                if (BH[j]) atomicAdd(&bucket_count[j], (unsigned long long)BH[j]);
        }
    }
}

hipError_t launch_group_prep(hipStream_t st, const int32_t* gkeys, int64_t n, const SpGroups* gp, uint8_t* need,
                             uint32_t* hist, uint32_t* err, uint64_t* bucket_count, int nbuckets, int32_t* cells,
                             uint32_t* tile_off) {
    if (n <= 0) return hipSuccess;
    const size_t lds = nbuckets <= kMmLdsBuckets ? sizeof(uint32_t) * (size_t)(nbuckets > 0 ? nbuckets : 1) : 0;
    static bool attr = false;
    if (!attr) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_group_prep),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(sizeof(uint32_t) * kMmLdsBuckets));
        if (e != hipSuccess) return e;
        attr = true;
    }
    const int64_t chunk = mm_chunk(n);
    hipLaunchKernelGGL(k_group_prep, dim3((unsigned)sp_tiles(n, chunk)), dim3(kMmThreads), lds, st, gkeys, n, gp,
                       need, hist, err, reinterpret_cast<unsigned long long*>(bucket_count), nbuckets, cells,
                       nbuckets <= kMmLdsBuckets ? tile_off : nullptr, chunk);
    return hipGetLastError();
}

// Scatter the pairs into bucket order: per-workgroup bucket counts reserve one range per bucket
// (one global atomic per workgroup and bucket), lanes take slots with LDS atomics.  Each thread
// handles 4 elements per step (4 independent load -> LDS atomic -> store chains), and the
// reserved 64-bit destinations sit in LDS, so the scatter never waits on a global load.
constexpr int kMmUnroll = 4;
__global__ __launch_bounds__(kMmThreads) void k_mm_scatter(const int32_t* __restrict__ gkeys,
                                                           const uint16_t* __restrict__ gbins, int64_t n,
                                                           const SpGroups* __restrict__ gp,
                                                           const uint64_t* __restrict__ bucket_base,
                                                           unsigned long long* __restrict__ cursor, int nbuckets,
                                                           uint64_t* __restrict__ pairs,
                                                           const int32_t* __restrict__ cells_in,
                                                           const uint32_t* __restrict__ tile_off, int64_t chunk) {
    if (gp->status) return;
    __shared__ int64_t S[kMaxGroups + 1];
    extern __shared__ uint64_t dyn64[];  // dst[nbuckets] (u64), cnt[nbuckets] (u32): dynamic, see launch
    uint64_t* dstb = dyn64;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(dyn64 + nbuckets);
    const int rows = gp->rows, zero = gp->zero;
    const bool lds_b = nbuckets <= kMmLdsBuckets;
    load_starts(gp, S);
    if (lds_b)
        for (int j = threadIdx.x; j < nbuckets; j += kMmThreads) cnt[j] = 0;
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * chunk, c1 = std::min<int64_t>(n, c0 + chunk);
    // cell of (element i, row r): from k_group_prep's table when it kept one, else hashed again
    auto cell_of = [&](int g, int r, int64_t i, int32_t key) -> int64_t {
        return cells_in ? (int64_t)cells_in[(int64_t)r * n + i] : mm_cell(gp, g, r, key);
    };
    if (lds_b && tile_off) {  // ranges reserved by k_group_prep
        const uint32_t* row = tile_off + (int64_t)blockIdx.x * nbuckets;
        for (int j = threadIdx.x; j < nbuckets; j += kMmThreads) dstb[j] = bucket_base[j] + row[j];
        __syncthreads();
    } else if (lds_b) {
        for (int64_t base = c0; base < c1; base += kMmUnroll * kMmThreads) {
#pragma unroll
            for (int u = 0; u < kMmUnroll; u++) {
                const int64_t i = base + u * kMmThreads + threadIdx.x;
                if (i >= c1) break;
                const int g = cells_in ? 0 : group_of_elem(S, i);
                const int32_t key = cells_in ? 0 : gkeys[i];
                for (int r = 0; r < rows; r++) atomicAdd(&cnt[(int)(cell_of(g, r, i, key) >> kMmBucketBits)], 1u);
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < nbuckets; j += kMmThreads) {
            dstb[j] = cnt[j] ? bucket_base[j] + atomicAdd(&cursor[j], (unsigned long long)cnt[j]) : 0ull;
            cnt[j] = 0;
        }
        __syncthreads();
    }
    if (lds_b && tile_off && cells_in) {
        // The common path, batched for memory-level parallelism: kMmBatch elements' keys, bins and
        // cells are loaded together (indices clamped into the tile), then ranked and stored.
        for (int64_t base = c0; base < c1; base += kMmBatch * kMmThreads) {
            int32_t key[kMmBatch], bin[kMmBatch];
            int64_t idx[kMmBatch];
#pragma unroll
            for (int u = 0; u < kMmBatch; u++) {
                const int64_t i = base + u * kMmThreads + threadIdx.x;
                idx[u] = i < c1 ? i : c1 - 1;
                key[u] = gkeys[idx[u]];
                bin[u] = gbins[idx[u]];
            }
            for (int r = 0; r < rows; r++) {
                int32_t cell[kMmBatch];
#pragma unroll
                for (int u = 0; u < kMmBatch; u++) cell[u] = cells_in[(int64_t)r * n + idx[u]];
#pragma unroll
                for (int u = 0; u < kMmBatch; u++) {
                    if (base + u * kMmThreads + threadIdx.x >= c1) continue;
                    const int b = cell[u] >> kMmBucketBits;
                    pairs[dstb[b] + atomicAdd(&cnt[b], 1u)] = mm_pair(key[u], bin[u], zero, cell[u]);
                }
            }
        }
    } else {
        for (int64_t base = c0; base < c1; base += kMmUnroll * kMmThreads) {
#pragma unroll
            for (int u = 0; u < kMmUnroll; u++) {
                const int64_t i = base + u * kMmThreads + threadIdx.x;
                if (i >= c1) break;
                const int g = cells_in ? 0 : group_of_elem(S, i);
                const int32_t key = gkeys[i], bin = gbins[i];
                for (int r = 0; r < rows; r++) {
                    const int64_t cell = cell_of(g, r, i, key);
                    const int b = (int)(cell >> kMmBucketBits);
                    const uint64_t dst = lds_b ? dstb[b] + atomicAdd(&cnt[b], 1u)
                                               : bucket_base[b] + (uint64_t)atomicAdd(&cursor[b], 1ull);
                    pairs[dst] = mm_pair(key, bin, zero, cell);
                }
            }
        }
    }
    if (lds_b && tile_off) {  // fill each range's padding (k_group_prep reserved mm_pad(count) slots)
        __syncthreads();
        for (int j = threadIdx.x; j < nbuckets * 16; j += kMmThreads) {
            const uint32_t c = cnt[j >> 4], slot = c + (uint32_t)(j & 15);
            if (c && slot < mm_pad(c)) pairs[dstb[j >> 4] + slot] = kMmNoPair;
        }
    }
}


// LDS-staged scatter (the common case: cells kept by k_group_prep, reserved ranges, at most
// kStageBuckets buckets).  The tile is cut into chunks of up to 8 pairs per thread; each chunk is
// ranked per bucket (LDS atomics), counting-sorted by bucket into LDS and stored bucket run by
// bucket run, so the pair stores go out as runs of consecutive addresses instead of one random
// 8-byte store per lane.  The next chunk's loads are issued before the current chunk's LDS phases.
constexpr int kStageBuckets = 4096;

template <int T>
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t v, uint32_t* sh, uint32_t& total) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(inc, off, 64);
        if (lane >= off) inc += y;
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < T / 64; j++) {
        const uint32_t x = sh[j];
        before += j < w ? x : 0u;
        tot += x;
    }
    total = tot;
    return before + inc - v;
}

// PAIR: uint64_t (key-carrying pairs) or uint32_t (narrow pairs, SpGroups.mm_narrow).
template <int T, typename PAIR>
__device__ __forceinline__ void mm_scatter_staged_body(const int32_t* __restrict__ gkeys,
                                                       const uint16_t* __restrict__ gbins, int64_t n,
                                                       const SpGroups* __restrict__ gp,
                                                       const uint64_t* __restrict__ bucket_base, int nbuckets,
                                                       PAIR* __restrict__ pairs, const int32_t* __restrict__ cells_in,
                                                       const uint32_t* __restrict__ tile_off, uint64_t* dyn64,
                                                       uint32_t* scan_sh, int64_t chunk) {
    constexpr bool kNarrow = sizeof(PAIR) == 4;
    constexpr int kStage = 8 * T;
    // LDS: dstb[nb] u64 | stage[kStage] PAIR | lc[nb] u32 | lofs[nb + 1] u32 | sb[kStage] u16
    uint64_t* dstb = dyn64;
    PAIR* stage = reinterpret_cast<PAIR*>(dstb + nbuckets);
    uint32_t* lc = reinterpret_cast<uint32_t*>(stage + kStage);
    uint32_t* lofs = lc + nbuckets;
    uint16_t* sb = reinterpret_cast<uint16_t*>(lofs + nbuckets + 1);
    const int t = threadIdx.x, rows = gp->rows, zero = gp->zero;
    const uint32_t* row = tile_off + (int64_t)blockIdx.x * nbuckets;
    for (int j = t; j < nbuckets; j += T) {
        dstb[j] = bucket_base[j] + row[j];
        lc[j] = 0;
    }
    const int64_t c0 = (int64_t)blockIdx.x * chunk, c1 = std::min<int64_t>(n, c0 + chunk);
    const int et = 8 / rows;  // elements per thread per chunk: et * rows <= 8 pairs each
    const int np = et * rows;
    const int64_t step = (int64_t)et * T;
    constexpr int kPer = (kStageBuckets + T - 1) / T;
    int32_t nk[8], nbn[8], nc[8];  // the next chunk's loads
    auto load = [&](int64_t base) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int u = k / rows, r = k - u * rows;
            const int64_t i = base + (int64_t)u * T + t;
            nc[k] = -1;
            if (k < np && i < c1) {
                nc[k] = cells_in[(int64_t)r * n + i];
                if constexpr (!kNarrow) nk[k] = gkeys[i];
                nbn[k] = gbins[i];
            }
        }
    };
    load(c0);
    __syncthreads();
    for (int64_t base = c0; base < c1; base += step) {
        PAIR pv[8];
        int32_t bk[8];
        uint32_t rk[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            bk[k] = nc[k] >= 0 ? nc[k] >> kMmBucketBits : -1;
            if (bk[k] >= 0) {
                if constexpr (kNarrow) pv[k] = mm_pair32(nbn[k], zero, nc[k]);
                else pv[k] = mm_pair(nk[k], nbn[k], zero, nc[k]);
            }
        }
        if (base + step < c1) load(base + step);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (bk[k] >= 0) rk[k] = atomicAdd(&lc[bk[k]], 1u);
        __syncthreads();
        // exclusive scan of the chunk's bucket counts
        uint32_t loc[kPer], sum = 0;
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int j = t * kPer + q;
            loc[q] = j < nbuckets ? lc[j] : 0u;
            sum += loc[q];
        }
        uint32_t total;
        uint32_t run = block_excl_scan_u32<T>(sum, scan_sh, total);
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int j = t * kPer + q;
            if (j < nbuckets) lofs[j] = run;
            run += loc[q];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (bk[k] >= 0) {
                const uint32_t q = lofs[bk[k]] + rk[k];
                stage[q] = pv[k];
                sb[q] = (uint16_t)bk[k];
            }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t q = (uint32_t)(u * T + t);
            if (q < total) {
                const int b = sb[q];
                pairs[dstb[b] + (q - lofs[b])] = stage[q];
            }
        }
        __syncthreads();
        for (int j = t; j < nbuckets; j += T)
            if (lc[j]) {
                dstb[j] += lc[j];
                lc[j] = 0;
            }
        __syncthreads();
    }
    // padding of each reserved range (mm_pad(count) slots): from the range's end up to the pad
    constexpr int kPadMax = kNarrow ? 32 : 16;
    for (int j = t; j < nbuckets * kPadMax; j += T) {
        const int bb = j / kPadMax;
        const uint64_t b0 = bucket_base[bb] + row[bb], e = dstb[bb];
        const uint64_t c = e - b0, slot = e + (uint64_t)(j % kPadMax);
        if (c && slot < b0 + mm_pad((uint32_t)c, kNarrow)) pairs[slot] = kNarrow ? (PAIR)kMmNoPair32 : (PAIR)kMmNoPair;
    }
}

template <int T>
__global__ __launch_bounds__(T) void k_mm_scatter_staged(const int32_t* __restrict__ gkeys,
                                                         const uint16_t* __restrict__ gbins, int64_t n,
                                                         const SpGroups* __restrict__ gp,
                                                         const uint64_t* __restrict__ bucket_base, int nbuckets,
                                                         void* __restrict__ pairs,
                                                         const int32_t* __restrict__ cells_in,
                                                         const uint32_t* __restrict__ tile_off, int64_t chunk) {
    if (gp->status) return;
    extern __shared__ uint64_t dyn64[];
    __shared__ uint32_t scan_sh[T / 64];
    if (gp->mm_narrow)
        mm_scatter_staged_body<T, uint32_t>(gkeys, gbins, n, gp, bucket_base, nbuckets,
                                            static_cast<uint32_t*>(pairs), cells_in, tile_off, dyn64, scan_sh, chunk);
    else
        mm_scatter_staged_body<T, uint64_t>(gkeys, gbins, n, gp, bucket_base, nbuckets,
                                            static_cast<uint64_t*>(pairs), cells_in, tile_off, dyn64, scan_sh, chunk);
}
#ifndef SKML_STAGE_THREADS
#define SKML_STAGE_THREADS 512
#endif
constexpr int kStageThreads = SKML_STAGE_THREADS;
inline size_t staged_lds(int nbuckets) {
    return (sizeof(uint64_t) + sizeof(uint16_t)) * 8 * kStageThreads + 16 * (size_t)nbuckets + 4;
}

bool mm_scatter_staged(bool cells, bool reserved, int nbuckets) {
    return cells && reserved && nbuckets <= kStageBuckets;
}

hipError_t launch_mm_scatter(hipStream_t st, const int32_t* gkeys, const uint16_t* gbins, int64_t n,
                             const SpGroups* gp, const uint64_t* bucket_base, uint64_t* cursor, int nbuckets,
                             void* pairs_v, const int32_t* cells, const uint32_t* tile_off) {
    uint64_t* pairs = static_cast<uint64_t*>(pairs_v);  // the unstaged scatter: key-carrying pairs only
    if (n <= 0) return hipSuccess;
    const int64_t chunk = mm_chunk(n);
    if (mm_scatter_staged(cells != nullptr, tile_off != nullptr, nbuckets)) {
        static bool attr_s = false;
        if (!attr_s) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mm_scatter_staged<kStageThreads>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)staged_lds(kStageBuckets));
            if (e != hipSuccess) return e;
            attr_s = true;
        }
        hipLaunchKernelGGL(k_mm_scatter_staged<kStageThreads>, dim3((unsigned)sp_tiles(n, chunk)),
                           dim3(kStageThreads), staged_lds(nbuckets), st, gkeys, gbins, n, gp, bucket_base, nbuckets,
                           pairs_v, cells, tile_off, chunk);
        return hipGetLastError();
    }
    constexpr size_t kPer = sizeof(uint64_t) + sizeof(uint32_t);
    const size_t lds = nbuckets <= kMmLdsBuckets ? kPer * (size_t)(nbuckets > 0 ? nbuckets : 1) : 0;
    static bool attr = false;
    if (!attr) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mm_scatter),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kPer * kMmLdsBuckets));
        if (e != hipSuccess) return e;
        attr = true;
    }
    hipLaunchKernelGGL(k_mm_scatter, dim3((unsigned)sp_tiles(n, chunk)), dim3(kMmThreads), lds, st, gkeys, gbins, n,
                       gp, bucket_base, reinterpret_cast<unsigned long long*>(cursor), nbuckets, pairs, cells,
                       nbuckets <= kMmLdsBuckets ? tile_off : nullptr, chunk);
    return hipGetLastError();
}

// One workgroup per bucket: LDS minimum per cell, then the int32 table cells (empty -> fill).
// Narrow pairs (SpGroups.mm_narrow) take 32-bit LDS minima over (distance, sign) for the whole
// bucket; key-carrying pairs take 64-bit minima, one 8192-cell sub-range after the other (each
// sub-range re-reads the bucket's pairs; this path only runs for groups on both sides of zeroIdx).
// tnar (may be nullptr): the exact narrow image of the table as well -- a cell's bin in 8 bits when
// the group table's bin_num <= 255, else in 16 bits when <= 65,535, the fill as the top code
// (2^W - 1); the payload's restore gathers from it and the exchange blob carries it
// (tnar_width_for).
__global__ __launch_bounds__(kMmThreads) void k_mm_bucket(const void* __restrict__ pairs_v,
                                                          const uint64_t* __restrict__ bucket_base,
                                                          const SpGroups* __restrict__ gp,
                                                          int32_t* __restrict__ table, void* __restrict__ tnar) {
    constexpr int kWords = kMmBucketCells / 2 > kMmSubCells ? kMmBucketCells / 2 : kMmSubCells;
    __shared__ unsigned long long cm64[kWords];  // u32 minima of the bucket, or u64 of a sub-range
    uint32_t* cm = reinterpret_cast<uint32_t*>(cm64);
    const int b = blockIdx.x;
    const int64_t ncells = gp->ncells;
    if (gp->status || ((int64_t)b << kMmBucketBits) >= ncells) return;
    const int32_t zero = gp->zero, fill = gp->fill;
    const uint64_t p0 = bucket_base[b], p1 = bucket_base[b + 1];
    const int64_t cell0 = (int64_t)b << kMmBucketBits;
    const int tw = tnar ? tnar_width_for(gp->bin_num) : 0;
    auto put = [&](int64_t cell, int32_t out) {
        table[cell] = out;
        if (tw == 8) static_cast<uint8_t*>(tnar)[cell] = out == fill ? (uint8_t)0xFF : (uint8_t)out;
        else if (tw == 16) static_cast<uint16_t*>(tnar)[cell] = out == fill ? (uint16_t)0xFFFF : (uint16_t)out;
    };
    if (gp->mm_narrow) {
        const uint32_t* pairs = static_cast<const uint32_t*>(pairs_v);
        for (int j = threadIdx.x; j < kMmBucketCells; j += kMmThreads) cm[j] = ~0u;
        __syncthreads();
        constexpr uint32_t kLo = (uint32_t)(kMmBucketCells - 1);
        constexpr int kB = 2 * kBucketBatch;  // half the bytes per pair: twice the pairs in flight
        for (uint64_t p = p0 + threadIdx.x; p < p1; p += kB * kMmThreads) {
            uint32_t v[kB];
#pragma unroll
            for (int u = 0; u < kB; u++) v[u] = p + u * kMmThreads < p1 ? pairs[p + u * kMmThreads] : kMmNoPair32;
#pragma unroll
            for (int u = 0; u < kB; u++)
                if (v[u] != kMmNoPair32) atomicMin(&cm[v[u] & kLo], v[u] >> kMmBucketBits);
        }
        __syncthreads();
        for (int j = threadIdx.x; j < kMmBucketCells && cell0 + j < ncells; j += kMmThreads) {
            const uint32_t v = cm[j];
            int32_t out = fill;
            if (v != ~0u) {
                const int32_t dist = (int32_t)(v >> 1);
                out = (v & 1u) ? zero - dist : zero + dist;
            }
            put(cell0 + j, out);
        }
        return;
    }
    const uint64_t* pairs = static_cast<const uint64_t*>(pairs_v);
    unsigned long long* cmin = cm64;
    constexpr uint64_t kLo = (uint64_t)(kMmBucketCells - 1), kSubLo = (uint64_t)(kMmSubCells - 1);
    for (int sub = 0; sub < kMmBucketCells / kMmSubCells; sub++) {
        const int64_t s0 = cell0 + (int64_t)sub * kMmSubCells;
        if (s0 >= ncells) break;
        if (sub) __syncthreads();  // the previous sub-range's cells are written
        for (int j = threadIdx.x; j < kMmSubCells; j += kMmThreads) cmin[j] = ~0ull;
        __syncthreads();
        for (uint64_t p = p0 + threadIdx.x; p < p1; p += kBucketBatch * kMmThreads) {
            uint64_t v[kBucketBatch];
#pragma unroll
            for (int u = 0; u < kBucketBatch; u++) v[u] = p + u * kMmThreads < p1 ? pairs[p + u * kMmThreads] : kMmNoPair;
#pragma unroll
            for (int u = 0; u < kBucketBatch; u++)
                if (v[u] != kMmNoPair && (int)((v[u] & kLo) >> kMmSubBits) == sub)
                    atomicMin(&cmin[v[u] & kSubLo], (unsigned long long)(v[u] & ~kLo));
        }
        __syncthreads();
        for (int j = threadIdx.x; j < kMmSubCells && s0 + j < ncells; j += kMmThreads) {
            const uint64_t v = cmin[j];
            int32_t out = fill;
            if (v != ~0ull) {
                const int32_t dist = (int32_t)(v >> 48);
                out = ((v >> 16) & 1u) ? zero - dist : zero + dist;
            }
            put(s0 + j, out);
        }
    }
}

hipError_t launch_mm_bucket(hipStream_t st, const void* pairs, const uint64_t* bucket_base, int nbuckets,
                            const SpGroups* gp, int32_t* table, void* tnar) {
    if (nbuckets <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_mm_bucket, dim3((unsigned)nbuckets), dim3(kMmThreads), 0, st, pairs, bucket_base, gp,
                       table, tnar);
    return hipGetLastError();
}

// SparseVectorCompressor.quantValues = Quantizer.getValues() (base/Quantizer.java:39-47) of the
// values' quantizer payload, on the device: the same double expressions the host evaluates after
// the encode's read-back, so the restore needs no upload of the table.
__global__ __launch_bounds__(256) void k_sp_qvalues(const uint8_t* __restrict__ qpayload, double* __restrict__ qv) {
    const skml_dense_header* h = reinterpret_cast<const skml_dense_header*>(qpayload);
    if (h->status != SKML_OK) return;
    const double* sp = reinterpret_cast<const double*>(qpayload + kHeaderBytes);
    const int B = h->bin_num, ns = B - 1;
    for (int b = (int)threadIdx.x; b < B && ns > 0; b += 256) {
        double v;
        if (b == 0) v = 0.5 * (h->min + sp[0]);
        else if (b == ns) v = 0.5 * (sp[ns - 1] + h->max);
        else v = 0.5 * (sp[b - 1] + sp[b]);
        qv[b] = v;
    }
}

hipError_t launch_sp_qvalues(hipStream_t st, const void* qpayload, double* qv) {
    hipLaunchKernelGGL(k_sp_qvalues, dim3(1), dim3(256), 0, st, static_cast<const uint8_t*>(qpayload), qv);
    return hipGetLastError();
}

// int32 cells from an exact narrow image (tnar_width_for): the top code back to the fill
__global__ __launch_bounds__(256) void k_widen_cells(const void* __restrict__ tn, int tw, int64_t ncells, int32_t fill,
                                                     int32_t* __restrict__ t32) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ncells; i += (int64_t)gridDim.x * 256) {
        const uint32_t v = tw == 8 ? static_cast<const uint8_t*>(tn)[i] : static_cast<const uint16_t*>(tn)[i];
        t32[i] = v == (tw == 8 ? 0xFFu : 0xFFFFu) ? fill : (int32_t)v;
    }
}

hipError_t launch_widen_cells(hipStream_t st, const void* tn, int tw, int64_t ncells, int32_t fill, int32_t* t32) {
    if (ncells <= 0) return hipSuccess;
    if (tw != 8 && tw != 16) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>(sp_tiles(ncells, 256 * 4), 4096);
    hipLaunchKernelGGL(k_widen_cells, dim3(grid), dim3(256), 0, st, tn, tw, ncells, fill, t32);
    return hipGetLastError();
}

// =============================================================================================
// Decode
// =============================================================================================
// Mask of the bits of word w that lie in unary-flag groups' flag ranges.
__device__ __forceinline__ uint64_t unary_mask(const SpGroups* gp, int64_t w) {
    const int64_t lo = w * 64, hi = lo + 64;
    uint64_t m = 0;
    for (int g = 0; g < gp->G; g++) {
        if (!gp->kind[g]) continue;
        const int64_t a = std::max(lo, gp->fb[g]), b = std::min(hi, gp->fb[g + 1]);
        if (a >= b) continue;
        const int la = (int)(a - lo), lb = (int)(b - lo);
        const uint64_t upto_b = lb >= 64 ? ~0ull : ((1ull << lb) - 1ull);
        m |= upto_b & ~((1ull << la) - 1ull);
    }
    return m;
}

__global__ __launch_bounds__(kSpThreads) void k_unary_count(const uint64_t* __restrict__ words, int64_t nwords,
                                                            const SpGroups* __restrict__ gp,
                                                            uint64_t* __restrict__ tile_sums) {
    __shared__ uint64_t sh[4];
    const int64_t w0 = (int64_t)blockIdx.x * kSpTile + threadIdx.x * 8;
    uint64_t c = 0;
    for (int j = 0; j < 8; j++) {
        const int64_t w = w0 + j;
        if (w < nwords) c += __popcll(~words[w] & unary_mask(gp, w));
    }
    uint64_t v[1] = {c}, tot[1];
    block_excl_scan<1>(v, tot, sh);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot[0];
}

hipError_t launch_unary_count(hipStream_t st, const uint64_t* flag_words, int64_t nwords,
                              const SpGroups* gp, uint64_t* tile_sums) {
    const int64_t tiles = sp_tiles(nwords, kSpTile);
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_unary_count, dim3((unsigned)tiles), dim3(kSpThreads), 0, st, flag_words, nwords, gp,
                       tile_sums);
    return hipGetLastError();
}

// Zero bit #r (over unary groups, in stream order) ends the flag of element
// gstart[g] + r - kind1_before[g]; its position is recorded in end_pos.
__global__ __launch_bounds__(kSpThreads) void k_unary_select(const uint64_t* __restrict__ words, int64_t nwords,
                                                             const SpGroups* __restrict__ gp,
                                                             const uint64_t* __restrict__ tile_base,
                                                             int64_t* __restrict__ end_pos) {
    __shared__ uint64_t sh[4];
    const int64_t w0 = (int64_t)blockIdx.x * kSpTile + threadIdx.x * 8;
    uint64_t z[8], c = 0;
    for (int j = 0; j < 8; j++) {
        const int64_t w = w0 + j;
        z[j] = w < nwords ? (~words[w] & unary_mask(gp, w)) : 0;
        c += __popcll(z[j]);
    }
    uint64_t v[1] = {c}, tot[1];
    block_excl_scan<1>(v, tot, sh);
    uint64_t r = tile_base[blockIdx.x] + v[0];
    int g = 0;
    for (int j = 0; j < 8; j++) {
        uint64_t m = z[j];
        while (m) {
            const int b = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const int64_t p = (w0 + j) * 64 + b;
            while (g + 1 < gp->G && gp->fb[g + 1] <= p) g++;
            const int64_t e = gp->gstart[g] + (int64_t)r - gp->kind1_before[g];
            if (e < gp->gstart[g + 1]) end_pos[e] = p;  // zeros past the last flag are padding
            r++;
        }
    }
}

hipError_t launch_unary_select(hipStream_t st, const uint64_t* flag_words, int64_t nwords,
                               const SpGroups* gp, const uint64_t* tile_base, int64_t* end_pos) {
    const int64_t tiles = sp_tiles(nwords, kSpTile);
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_unary_select, dim3((unsigned)tiles), dim3(kSpThreads), 0, st, flag_words, nwords, gp,
                       tile_base, end_pos);
    return hipGetLastError();
}

// BinaryUtils.getBits (binary/BinaryUtils.java:16-25): nbits (<= 32) read MSB-first.
__device__ __forceinline__ uint32_t get_bits(const uint64_t* words, int64_t nwords, int64_t off, int nbits) {
    if (nbits <= 0) return 0;
    const int64_t w = off >> 6;
    const int sh = (int)(off & 63);
    uint64_t lo = w < nwords ? words[w] : 0;
    uint64_t v = lo >> sh;
    if (sh + nbits > 64) {
        const uint64_t hi = (w + 1) < nwords ? words[w + 1] : 0;
        v |= hi << (64 - sh);
    }
    const uint32_t field = (uint32_t)(v & (nbits == 64 ? ~0ull : ((1ull << nbits) - 1ull)));
    return __brev(field) >> (32 - nbits);
}

// The same read from two words already in registers: off in [0, 64) is relative to w0 and
// off + nbits <= 128.
__device__ __forceinline__ uint32_t bits_of_window(uint64_t w0, uint64_t w1, int off, int nbits) {
    if (nbits <= 0) return 0;
    const uint64_t v = off ? (w0 >> off) | (w1 << (64 - off)) : w0;
    const uint32_t field = (uint32_t)(v & ((1ull << nbits) - 1ull));
    return __brev(field) >> (32 - nbits);
}
__device__ __forceinline__ uint64_t word_or_zero(const uint64_t* __restrict__ words, int64_t nwords, int64_t w) {
    return w < nwords ? words[w] : 0ull;
}

template <typename TN>
__device__ __forceinline__ void narrow_cells(const int32_t* __restrict__ t32, int64_t ncells, TN* __restrict__ tn,
                                             int64_t blk) {
    constexpr uint32_t kTop = (uint32_t)(TN)~(TN)0;
    const int64_t i0 = (blk * kSpThreads + threadIdx.x) * 4;
    if (i0 + 4 <= ncells) {
        const int4 v = *reinterpret_cast<const int4*>(t32 + i0);
        const int32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) tn[i0 + j] = (TN)((uint32_t)e[j] < kTop ? (uint32_t)e[j] : kTop);
    } else {
        for (int64_t i = i0; i < ncells; i++) tn[i] = (TN)((uint32_t)t32[i] < kTop ? (uint32_t)t32[i] : kTop);
    }
}
// The DeltaAdaptive bit lengths of elements i0 .. i0 + 7 (flag stream -> interval -> bits per
// delta) into l[], 0 past n; returns their sum.
__device__ __forceinline__ uint64_t dec_lens8(const uint64_t* __restrict__ fw, int64_t nfw,
                                              const int64_t* __restrict__ end_pos, int64_t n,
                                              const SpGroups* __restrict__ gp, const int64_t* S, int64_t i0,
                                              uint8_t (&l)[8]) {
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) l[j] = 0;
    int gf = i0 < n ? group_of_elem(S, i0) : 0;
    if (i0 + 8 <= n && i0 + 8 <= S[gf + 1] && !gp->kind[gf]) {
        // the common case: 8 fixed-width flags of one group, at most 40 contiguous bits: two word
        // loads instead of one or two per element
        const DeltaShape s = delta_shape(gp, gf);
        const int64_t b0 = gp->fb[gf] + (i0 - S[gf]) * s.nf;
        const int64_t w = b0 >> 6;
        const int sh = (int)(b0 & 63);
        const uint64_t w0 = word_or_zero(fw, nfw, w), w1 = word_or_zero(fw, nfw, w + 1);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int off = sh + j * s.nf;  // < 64 + 40
            const uint32_t f = off < 64 ? bits_of_window(w0, w1, off, s.nf) : bits_of_window(w1, 0ull, off - 64, s.nf);
            const int dl = s.bpi * ((int)f + 1);
            l[j] = (uint8_t)dl;
            sum += dl;
        }
    } else if (i0 < n) {
        int g = gf;
        DeltaShape s = delta_shape(gp, g);
        for (int j = 0; j < 8; j++) {
            const int64_t i = i0 + j;
            if (i >= n) break;
            while (i >= S[g + 1]) s = delta_shape(gp, ++g);
            int iv;
            if (!s.kind) {
                iv = (int)get_bits(fw, nfw, gp->fb[g] + (i - S[g]) * s.nf, s.nf) + 1;
            } else {
                const int64_t start = i == S[g] ? gp->fb[g] : end_pos[i - 1] + 1;
                iv = (int)(end_pos[i] - start);
            }
            const int dl = s.bpi * iv;
            l[j] = (uint8_t)dl;
            sum += dl;
        }
    }
    return sum;
}

__global__ __launch_bounds__(kSpThreads) void k_dec_lens(const uint64_t* __restrict__ fw, int64_t nfw,
                                                         const int64_t* __restrict__ end_pos, int64_t n,
                                                         const SpGroups* __restrict__ gp, uint8_t* __restrict__ dlen,
                                                         uint64_t* __restrict__ tile_sums, int64_t nlens,
                                                         NarrowJob nj) {
    if ((int64_t)blockIdx.x >= nlens) {  // the blocks past the lengths' tiles build the narrow table
        const int64_t b = (int64_t)blockIdx.x - nlens;
        if (nj.width == 8) narrow_cells<uint8_t>(nj.t32, nj.ncells, static_cast<uint8_t*>(nj.tn), b);
        else narrow_cells<uint16_t>(nj.t32, nj.ncells, static_cast<uint16_t*>(nj.tn), b);
        return;
    }
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ uint64_t sh[4];
    load_starts(gp, S);
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * kSpTile + threadIdx.x * 8;
    uint8_t l[8];
    const uint64_t sum = dec_lens8(fw, nfw, end_pos, n, gp, S, i0, l);
    if (i0 + 8 <= n) {  // one 8-byte store of the lengths
        uint64_t packed = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) packed |= (uint64_t)l[j] << (8 * j);
        *reinterpret_cast<uint64_t*>(dlen + i0) = packed;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (i0 + j < n) dlen[i0 + j] = l[j];
    }
    uint64_t v[1] = {sum}, tot[1];
    block_excl_scan<1>(v, tot, sh);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot[0];
}

hipError_t launch_dec_lens(hipStream_t st, const uint64_t* flag_words, int64_t n_flag_words,
                           const int64_t* end_pos, int64_t n, const SpGroups* gp, uint8_t* dlen,
                           uint64_t* tile_sums, NarrowJob nj) {
    const int64_t tiles = sp_tiles(n, kSpTile);
    if (tiles <= 0) return nj.tn ? launch_narrow_table(st, nj.t32, nj.ncells, nj.width, nj.tn) : hipSuccess;
    if (nj.tn && (reinterpret_cast<uintptr_t>(nj.t32) & 15) != 0) return hipErrorInvalidValue;
    const int64_t nn = nj.tn && nj.ncells > 0 ? sp_tiles(nj.ncells, (int64_t)kSpThreads * 4) : 0;
    hipLaunchKernelGGL(k_dec_lens, dim3((unsigned)(tiles + nn)), dim3(kSpThreads), 0, st, flag_words, n_flag_words,
                       end_pos, n, gp, dlen, tile_sums, tiles, nj);
    return hipGetLastError();
}

// The deltas of elements i0 .. i0 + 7 from their lengths l[] and the first one's bit offset
// `off` in the delta stream, stored to delta[]; returns their sum.
__device__ __forceinline__ uint64_t dec_deltas8(const uint64_t* __restrict__ dw, int64_t ndw, int64_t n, int64_t i0,
                                                int64_t off, const uint8_t (&l)[8], uint32_t* __restrict__ delta) {
    uint64_t dsum = 0;
    if (i0 + 8 <= n) {
        // the thread's 8 deltas are contiguous, at most 256 bits: five words loaded up front, each
        // field taken from the two words it straddles
        const int64_t w = off >> 6;
        uint64_t W[5];
#pragma unroll
        for (int q = 0; q < 5; q++) W[q] = word_or_zero(dw, ndw, w + q);
        int r = (int)(off & 63);
        uint32_t d[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int q = r >> 6, o = r & 63;
            const uint64_t lo = q == 0 ? W[0] : q == 1 ? W[1] : q == 2 ? W[2] : q == 3 ? W[3] : W[4];
            const uint64_t hi = q == 0 ? W[1] : q == 1 ? W[2] : q == 2 ? W[3] : q == 3 ? W[4] : 0ull;
            d[j] = bits_of_window(lo, hi, o, l[j]);
            dsum += d[j];
            r += l[j];
        }
        *reinterpret_cast<uint4*>(delta + i0) = make_uint4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<uint4*>(delta + i0 + 4) = make_uint4(d[4], d[5], d[6], d[7]);
    } else {
        for (int j = 0; j < 8; j++) {
            if (i0 + j >= n) break;
            const uint32_t d = get_bits(dw, ndw, off, l[j]);
            delta[i0 + j] = d;
            dsum += d;
            off += l[j];
        }
    }
    return dsum;
}

__global__ __launch_bounds__(kSpThreads) void k_dec_deltas(const uint64_t* __restrict__ dw, int64_t ndw,
                                                           const uint8_t* __restrict__ dlen, int64_t n,
                                                           const uint64_t* __restrict__ tile_base,
                                                           uint32_t* __restrict__ delta, uint64_t* __restrict__ tile_sums) {
    __shared__ uint64_t sh[4];
    const int64_t i0 = (int64_t)blockIdx.x * kSpTile + threadIdx.x * 8;
    uint8_t l[8];
    uint64_t sum = 0;
    if (i0 + 8 <= n) {  // one 8-byte load of the lengths
        const uint64_t pk = *reinterpret_cast<const uint64_t*>(dlen + i0);
#pragma unroll
        for (int j = 0; j < 8; j++) l[j] = (uint8_t)(pk >> (8 * j));
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) l[j] = i0 + j < n ? dlen[i0 + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) sum += l[j];
    uint64_t v[1] = {sum}, tot[1];
    block_excl_scan<1>(v, tot, sh);
    const uint64_t dsum = dec_deltas8(dw, ndw, n, i0, (int64_t)(tile_base[blockIdx.x] + v[0]), l, delta);
    uint64_t v2[1] = {dsum}, tot2[1];
    block_excl_scan<1>(v2, tot2, sh);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot2[0];
}

#ifdef SKML_AB  // A/B form, measured slower (profiles/ab/r05_dec_lookback.txt)
// Lengths and deltas in one pass: each tile (taken in ticket order) computes its lengths in
// registers, takes its first bit offset in the delta stream by a decoupled look-back over the
// tiles' bit totals (the compaction's scheme), and extracts its deltas -- no length array written
// and read back, no tile scan in between.  Extra blocks past the tiles build the narrow table.
__device__ __forceinline__ uint64_t lookback_excl(uint64_t* status, int64_t tile, uint64_t total, int lane) {
    uint64_t excl = 0;
    if (tile == 0) {
        if (lane == 0) st_status(&status[0], kStPre | total);
        return 0;
    }
    if (lane == 0) st_status(&status[tile], kStAgg | total);
    int64_t p = tile - 1;
    while (true) {
        const int64_t idx = p - lane;
        uint64_t sv = idx >= 0 ? ld_status(&status[idx]) : kStPre;  // before tile 0: prefix 0
        while (__ballot((sv & ~kStMask) == 0)) {
            __builtin_amdgcn_s_sleep(1);
            if ((sv & ~kStMask) == 0) sv = ld_status(&status[idx]);
        }
        const uint64_t pre = __ballot((sv & ~kStMask) == kStPre);
        const int stop = pre ? __ffsll((unsigned long long)pre) - 1 : 63;  // nearest prefix
        uint64_t contrib = lane <= stop ? (sv & kStMask) : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) contrib += __shfl_xor(contrib, off, 64);
        excl += contrib;
        if (pre) break;
        p -= 64;
    }
    if (lane == 0) st_status(&status[tile], kStPre | (excl + total));
    return excl;
}
__global__ __launch_bounds__(kSpThreads) void k_dec_lens_deltas(const uint64_t* __restrict__ fw, int64_t nfw,
                                                                const int64_t* __restrict__ end_pos, int64_t n,
                                                                const SpGroups* __restrict__ gp,
                                                                const uint64_t* __restrict__ dw, int64_t ndw,
                                                                uint32_t* __restrict__ delta,
                                                                uint64_t* __restrict__ tile_sums, uint64_t* status,
                                                                uint64_t* status2, unsigned* ticket, int64_t nlens,
                                                                NarrowJob nj) {
    if ((int64_t)blockIdx.x >= nlens) {  // the blocks past the tiles build the narrow table
        const int64_t b = (int64_t)blockIdx.x - nlens;
        if (nj.width == 8) narrow_cells<uint8_t>(nj.t32, nj.ncells, static_cast<uint8_t*>(nj.tn), b);
        else narrow_cells<uint16_t>(nj.t32, nj.ncells, static_cast<uint16_t*>(nj.tn), b);
        return;
    }
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ uint64_t sh[4];
    __shared__ int64_t s_tile;
    __shared__ uint64_t s_excl;
    load_starts(gp, S);
    if (threadIdx.x == 0) s_tile = (int64_t)atomicAdd(ticket, 1u);  // tiles in arrival order
    __syncthreads();
    const int64_t tile = s_tile;
    const int64_t i0 = tile * kSpTile + threadIdx.x * 8;
    uint8_t l[8];
    const uint64_t sum = dec_lens8(fw, nfw, end_pos, n, gp, S, i0, l);
    uint64_t v[1] = {sum}, tot[1];
    block_excl_scan<1>(v, tot, sh);
    if (threadIdx.x < 64) {
        const uint64_t excl = lookback_excl(status, tile, tot[0], (int)threadIdx.x);
        if (threadIdx.x == 0) s_excl = excl;
    }
    __syncthreads();
    const uint64_t dsum = dec_deltas8(dw, ndw, n, i0, (int64_t)(s_excl + v[0]), l, delta);
    uint64_t v2[1] = {dsum}, tot2[1];
    block_excl_scan<1>(v2, tot2, sh);
    if (status2) {  // the tiles' delta prefixes too (a second look-back): tile_sums = the exclusive scan
        if (threadIdx.x < 64) {
            const uint64_t excl2 = lookback_excl(status2, tile, tot2[0], (int)threadIdx.x);
            if (threadIdx.x == 0) {
                tile_sums[tile] = excl2;
                if (tile == nlens - 1) tile_sums[nlens] = excl2 + tot2[0];
            }
        }
    } else if (threadIdx.x == 0) {
        tile_sums[tile] = tot2[0];
    }
}

hipError_t launch_dec_lens_deltas(hipStream_t st, const uint64_t* flag_words, int64_t n_flag_words,
                                  const int64_t* end_pos, int64_t n, const SpGroups* gp,
                                  const uint64_t* delta_words, int64_t n_delta_words, uint32_t* delta,
                                  uint64_t* tile_sums, uint64_t* status, NarrowJob nj, bool scan_sums) {
    const int64_t tiles = sp_tiles(n, kSpTile);
    if (tiles <= 0) return nj.tn ? launch_narrow_table(st, nj.t32, nj.ncells, nj.width, nj.tn) : hipSuccess;
    if (nj.tn && (reinterpret_cast<uintptr_t>(nj.t32) & 15) != 0) return hipErrorInvalidValue;
    // statuses of the bit offsets, the ticket, statuses of the delta prefixes
    hipError_t e = hipMemsetAsync(status, 0, sizeof(uint64_t) * (size_t)(2 * tiles + 2), st);
    if (e != hipSuccess) return e;
    const int64_t nn = nj.tn && nj.ncells > 0 ? sp_tiles(nj.ncells, (int64_t)kSpThreads * 4) : 0;
    hipLaunchKernelGGL(k_dec_lens_deltas, dim3((unsigned)(tiles + nn)), dim3(kSpThreads), 0, st, flag_words,
                       n_flag_words, end_pos, n, gp, delta_words, n_delta_words, delta, tile_sums, status,
                       scan_sums ? status + tiles + 2 : nullptr, reinterpret_cast<unsigned*>(status + tiles), tiles,
                       nj);
    return hipGetLastError();
}
#endif  // SKML_AB


hipError_t launch_dec_deltas(hipStream_t st, const uint64_t* delta_words, int64_t n_delta_words,
                             const uint8_t* dlen, int64_t n, const SpGroups* gp,
                             const uint64_t* tile_base, uint32_t* delta, uint64_t* tile_sums) {
    (void)gp;
    const int64_t tiles = sp_tiles(n, kSpTile);
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_dec_deltas, dim3((unsigned)tiles), dim3(kSpThreads), 0, st, delta_words, n_delta_words,
                       dlen, n, tile_base, delta, tile_sums);
    return hipGetLastError();
}

// Exclusive delta prefix at each group's first element: tile base + the in-tile partial sum.
__global__ __launch_bounds__(kSpThreads) void k_group_prefix(const uint32_t* __restrict__ delta, int64_t n,
                                                             const SpGroups* __restrict__ gp,
                                                             const uint64_t* __restrict__ tile_base,
                                                             uint64_t* __restrict__ gpre) {
    __shared__ uint64_t sh[4];
    const int g = blockIdx.x;
    const int64_t s0 = gp->gstart[g];
    const int64_t tile = s0 / kSpTile, lo = tile * kSpTile;
    uint64_t sum = 0;
    for (int64_t i = lo + threadIdx.x; i < s0 && i < n; i += kSpThreads) sum += delta[i];
    uint64_t v[1] = {sum}, tot[1];
    block_excl_scan<1>(v, tot, sh);
    if (threadIdx.x == 0) gpre[g] = (s0 < n ? tile_base[tile] : 0) + tot[0];
}

hipError_t launch_group_prefix(hipStream_t st, const uint32_t* delta, int64_t n, const SpGroups* gp, int G,
                               const uint64_t* tile_base, uint64_t* gpre) {
    hipLaunchKernelGGL(k_group_prefix, dim3(G), dim3(kSpThreads), 0, st, delta, n, gp, tile_base, gpre);
    return hipGetLastError();
}

// A narrow image of the int32 MinMax tables for the query: values in [0, 2^W - 1) exactly, the
// rest (the fill of empty cells, and the top code itself) as the sentinel 2^W - 1, which sends the
// query back to the int32 cell.  A valid payload only queries inserted cells, so at W = 8 (binNum
// <= 256) the int32 table is read for bin 255 alone.  At C3 a group's two rows are 2 MB of bytes:
// with each group's tiles on one XCD (k_dec_keys) the gathers hit that XCD's 4 MB L2.
template <typename TN>
__global__ __launch_bounds__(kSpThreads) void k_narrow_table(const int32_t* __restrict__ t32, int64_t ncells,
                                                             TN* __restrict__ tn) {
    narrow_cells<TN>(t32, ncells, tn, blockIdx.x);
}

hipError_t launch_narrow_table(hipStream_t st, const int32_t* t32, int64_t ncells, int width, void* tn) {
    if (ncells <= 0) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(t32) & 15) != 0) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)sp_tiles(ncells, (int64_t)kSpThreads * 4);
    if (width == 8)
        hipLaunchKernelGGL(k_narrow_table<uint8_t>, dim3(grid), dim3(kSpThreads), 0, st, t32, ncells,
                           static_cast<uint8_t*>(tn));
    else
        hipLaunchKernelGGL(k_narrow_table<uint16_t>, dim3(grid), dim3(kSpThreads), 0, st, t32, ncells,
                           static_cast<uint16_t*>(tn));
    return hipGetLastError();
}

// Workgroup -> tile of k_dec_keys: each tile belongs to the group holding its first element, and
// the tiles of group g go to workgroups b with b % 8 == g % 8, which the dispatcher deals to one XCD
// (speed only: any placement gives the same result).  -1: an idle workgroup.
__device__ __forceinline__ int64_t dec_tile_of_block(const int64_t* S, int G, int64_t b) {
    const int x = (int)(b & 7);
    int64_t j = b >> 3;
    for (int g = x; g < G; g += 8) {
        const int64_t t0 = sp_tiles(S[g], kSpTile), t1 = sp_tiles(S[g + 1], kSpTile);
        if (j < t1 - t0) return t0 + j;
        j -= t1 > t0 ? t1 - t0 : 0;
    }
    return -1;
}

// keys: group-restarted prefix sums of the deltas (Java int wrap); bins: MinMaxSketch.query
// (MinMaxSketch.java:64-73): the row value farthest from zero, the first row on ties.  TN: the
// narrow table's cell type (int32_t: the int32 table itself).  512 threads per 2,048-element tile,
// 4 consecutive elements per thread (16-byte delta loads and key stores).
constexpr int kDecThreads = 512;
static_assert(kDecThreads * 4 == kSpTile, "dec_keys tile");
// MODE 1: the default shape (2 rows), tiles inside one group only (a tile across a group edge
// returns at once): both rows' hashes fixed at compile time by a switch on the group's hash ids,
// 8 gathers in flight per thread, cells as 32-bit offsets.  MODE 0: any shape and any tile, one
// row at a time with a per-lane hash id; it runs the whole grid for other shapes, or only the
// edge tiles (`edges`, at most one per group edge) after a MODE 1 launch.  Keeping the two apart
// keeps MODE 1's registers at what its own code needs.
struct DecEdgeTiles {
    int64_t t[kMaxGroups];
    int n;  // 0: every tile (dec_tile_of_block)
};
// NT: the delta stream and the key / bin stores nontemporal, so they pass L2 without evicting the
// table the gathers read.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef int32_t i32x4_t __attribute__((ext_vector_type(4)));
// One tile of k_dec_keys from its preloaded deltas `d` and base `tb` (tile_base[tile]).  sh: one
// u64 per wave of LDS (the cross-wave prefix); a persistent caller alternates two of them.
template <typename TN, int MODE, bool NT>
__device__ __forceinline__ void dec_keys_tile(int64_t n, const SpGroups* __restrict__ gp,
                                              const uint64_t* __restrict__ gpre, const int32_t* __restrict__ table,
                                              const TN* __restrict__ tnar, int32_t* __restrict__ gkeys,
                                              int32_t* __restrict__ gbins, int nq, void* __restrict__ gbn,
                                              int bn_width, unsigned* __restrict__ err, const int64_t* S,
                                              uint64_t* sh, int64_t tile, const uint32_t (&d)[4], uint64_t tb,
                                              int tid, const RunBoundsOut& rb) {
    const int t = tid, lane = t & 63, w = t >> 6;
    const int64_t i0 = tile * kSpTile + t * 4;
    // the tile's exclusive prefix of the deltas (64-bit: a tile's deltas may pass 2^32)
    const uint64_t own = (uint64_t)d[0] + d[1] + d[2] + d[3];
    const uint64_t inc = wave_incl_u64(own, lane);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint64_t p = tb + inc - own;
#pragma unroll
    for (int j = 0; j < kDecThreads / 64; j++) p += j < w ? sh[j] : 0ull;
    if (i0 >= n) return;
    const uint64_t p_before = p;  // the deltas' prefix through element i0 - 1
    const int zero = gp->zero, rows = gp->rows;
    int32_t key[4], res[4];
    int grp[4];
    if constexpr (MODE == 1) {  // the tile's one group, workgroup-uniform
        const int g = __builtin_amdgcn_readfirstlane(group_of_elem(S, tile * kSpTile));
        const uint64_t gb = gpre[g];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            p += d[j];
            grp[j] = g;
            key[j] = (int32_t)(uint32_t)(p - gb);
            res[j] = zero;
        }
    } else {
        int g = group_of_elem(S, i0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t i = i0 + j;
            if (i < n)
                while (i >= S[g + 1]) g++;
            p += d[j];
            grp[j] = g;
            key[j] = (int32_t)(uint32_t)(p - gpre[g]);
            res[j] = zero;
        }
    }
    if (rb.bounds) {  // the runs' bounds (run_bounds16's rules), from the keys in hand
        const bool rs = rb.info != nullptr;  // Sort.merge's key ranges, else Gradient.sum's tiles
        const int64_t ld = rs ? kRsRanges + 1 : rb.ntiles + 1;
        bool bad = false;
        auto tile_of = [&](int32_t k) -> int64_t {
            if (rs) return (int64_t)(k >> kRsBits);
            return k < 0 ? 0 : std::min<int64_t>((int64_t)(k >> rb.tile_bits), rb.ntiles);
        };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t i = i0 + j;
            if (i >= n) break;
            const int g = grp[j];
            const int64_t lo = S[g], hi = S[g + 1];
            const int32_t k = key[j];
            const bool first = i == lo;
            // the element before, inside the same run when this one is not its first
            const int32_t prev = j > 0 ? key[j - 1] : (int32_t)(uint32_t)(p_before - gpre[g]);
            bool ok = true;
            if (rs) {  // the one-pass merge's regular input (else the merge rounds run)
                ok = !(k < 0 || k == INT32_MAX || (!first && k <= prev));
                bad |= !ok;
            } else {
                if (k < 0 || (int64_t)k >= rb.dim) bad = true;  // SparseDoubleGradient's bound check
                if (!first && k <= prev) bad = true;            // keys ascend strictly inside a run
            }
            if (ok) {
                const int64_t ti = tile_of(k), pt = first || (rs && prev < 0) ? -1 : tile_of(prev);
                int32_t* b = rb.bounds + (int64_t)g * ld;
                for (int64_t t = pt + 1; t <= ti; t++) b[t] = (int32_t)i;
                if (i == hi - 1) {
                    if (rs) {  // the run's last range ends at the run's end
                        b[ti + 1] = (int32_t)hi;
                        rb.info->tlast1[g] = (int32_t)ti + 1;
                        atomicMax(&rb.info->tmax1, (int32_t)ti + 1);
                    } else {
                        for (int64_t t = ti + 1; t <= rb.ntiles; t++) b[t] = (int32_t)hi;
                    }
                }
            }
        }
        if (bad) atomicOr(rs ? &rb.info->irregular : err, 1u);
    }
    constexpr uint32_t kTop = sizeof(TN) == 4 ? 0u : (uint32_t)(TN)~(TN)0;
    auto cell_of = [&](int j, int r) -> int64_t {
        const int gj = grp[j];
        const int32_t cols = gp->cols[gj];
        return i0 + j < n ? gp->tab_off[gj] + (int64_t)r * cols +
                                java_hash_fm(gp->hash_ids[gj][r], key[j], cols, gp->inv_cols[gj])
                          : -1;
    };
    auto gather = [&](int64_t idx) -> int32_t {
        if constexpr (sizeof(TN) == 4) return idx >= 0 ? table[idx] : zero;
        else return idx >= 0 ? (int32_t)tnar[idx] : zero;
    };
    // MinMaxSketch.query: the strictly farther value wins, ties keep the earlier row
    auto take = [&](int j, int32_t tv) {
        if ((int32_t)((uint32_t)mm_dist(tv, zero) - (uint32_t)mm_dist(res[j], zero)) > 0) res[j] = tv;
    };
    if constexpr (MODE == 1) {
        // both rows' 8 cells hashed, all 8 gathers in flight at once (the query is bound by the
        // gathers' L2 latency); the host runs this form only while every cell index is below
        // 2^32 - 1
        const int g0 = grp[0];  // the tile's one group
        const int64_t tb = gp->tab_off[g0];
        const int32_t cols = gp->cols[g0];
        const double inv = gp->inv_cols[g0];
        const DivU32 dvc = divu32_make((uint32_t)cols);
        const auto dv = [&](uint32_t h) { return java_mod((int32_t)h, cols, dvc); };
        const TN* tnb = tnar + tb;
        const int32_t* t32b = table ? table + tb : nullptr;  // nullptr: tnar is exact (top code = fill)
        uint32_t rel[2][4];
        int32_t tv[2][4];
#pragma unroll
        for (int r = 0; r < 2; r++) {  // a row's 4 gathers leave before the next row is hashed
            const int id = __builtin_amdgcn_readfirstlane(gp->hash_ids[g0][r]);
            const int64_t row0 = (int64_t)r * cols;
            switch (id) {
                case 0: dec_row_cells<0>(key, i0, n, row0, cols, inv, dv, rel[r]); break;
                case 1: dec_row_cells<1>(key, i0, n, row0, cols, inv, dv, rel[r]); break;
                case 2: dec_row_cells<2>(key, i0, n, row0, cols, inv, dv, rel[r]); break;
                case 3: dec_row_cells<3>(key, i0, n, row0, cols, inv, dv, rel[r]); break;
                case 4: dec_row_cells<4>(key, i0, n, row0, cols, inv, dv, rel[r]); break;
                case 5: dec_row_cells<5>(key, i0, n, row0, cols, inv, dv, rel[r]); break;
                case 6: dec_row_cells<6>(key, i0, n, row0, cols, inv, dv, rel[r]); break;
                default: dec_row_cells<7>(key, i0, n, row0, cols, inv, dv, rel[r]); break;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
#ifdef SKML_ABLATE_DEC_GATHER  // timing ablation only (wrong bins): the table gathers priced
                tv[r][j] = (int32_t)(rel[r][j] & 0x3Fu);
                continue;
#endif
                if constexpr (sizeof(TN) == 4) tv[r][j] = t32b[rel[r][j]];
                else tv[r][j] = (int32_t)tnb[rel[r][j]];
            }
        }
        if constexpr (sizeof(TN) < 4) {
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int j = 0; j < 4; j++)  // the top code: the cell's int32 value, or the fill
                    if ((uint32_t)tv[r][j] == kTop) tv[r][j] = t32b ? t32b[rel[r][j]] : gp->fill;
        }
#ifdef SKML_ABLATE_DEC_HASH  // (the wrong cells may be empty ones: keep the bins inside quantValues)
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int j = 0; j < 4; j++) tv[r][j] &= 0x3F;
#endif
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int j = 0; j < 4; j++) take(j, tv[r][j]);
    } else {
        for (int r = 0; r < rows; r++) {
            int64_t idx[4];
            int32_t tv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                idx[j] = cell_of(j, r);
                tv[j] = gather(idx[j]);
            }
            if constexpr (sizeof(TN) < 4) {
#pragma unroll
                for (int j = 0; j < 4; j++)  // the top code: the cell's int32 value, or the fill
                    if (idx[j] >= 0 && (uint32_t)tv[j] == kTop) tv[j] = table ? table[idx[j]] : gp->fill;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) take(j, tv[j]);
        }
    }
    const bool full = i0 + 4 <= n;
    if (gbn) {  // Gradient.sum's restore: narrow bins (the values come from quantValues in LDS later);
                // a bin outside the values is an error
        bool bad = false;
        uint32_t b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool ok = res[j] >= 0 && res[j] < nq;
            bad |= !ok && i0 + j < n;
            b[j] = ok ? (uint32_t)res[j] : 0u;
        }
        if (bad) atomicOr(err, 1u);
        if (bn_width == 1) {
            uint8_t* o = static_cast<uint8_t*>(gbn) + i0;
            if (full && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
                const uint32_t w4 = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
                if constexpr (NT) __builtin_nontemporal_store(w4, reinterpret_cast<uint32_t*>(o));
                else *reinterpret_cast<uint32_t*>(o) = w4;
            } else
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (i0 + j < n) o[j] = (uint8_t)b[j];
        } else {
            uint16_t* o = static_cast<uint16_t*>(gbn) + i0;
            if (full && (reinterpret_cast<uintptr_t>(o) & 7) == 0)
                *reinterpret_cast<uint2*>(o) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
            else
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (i0 + j < n) o[j] = (uint16_t)b[j];
        }
    }
    if (full && (reinterpret_cast<uintptr_t>(gkeys + i0) & 15) == 0) {
        if constexpr (NT) {
            const i32x4_t kv = {key[0], key[1], key[2], key[3]};
            __builtin_nontemporal_store(kv, reinterpret_cast<i32x4_t*>(gkeys + i0));
        } else {
            *reinterpret_cast<int4*>(gkeys + i0) = make_int4(key[0], key[1], key[2], key[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0 + j < n) gkeys[i0 + j] = key[j];
    }
    if (gbins) {
        if (full && (reinterpret_cast<uintptr_t>(gbins + i0) & 15) == 0) {
            *reinterpret_cast<int4*>(gbins + i0) = make_int4(res[0], res[1], res[2], res[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (i0 + j < n) gbins[i0 + j] = res[j];
        }
    }
}


template <typename TN, int MODE, bool NT = false>
__global__ __launch_bounds__(kDecThreads) void k_dec_keys(const uint32_t* __restrict__ delta, int64_t n,
                                                          const SpGroups* __restrict__ gp,
                                                          const uint64_t* __restrict__ tile_base,
                                                          const uint64_t* __restrict__ gpre,
                                                          const int32_t* __restrict__ table, const TN* __restrict__ tnar,
                                                          int32_t* __restrict__ gkeys, int32_t* __restrict__ gbins,
                                                          int nq, void* __restrict__ gbn, int bn_width,
                                                          unsigned* __restrict__ err, DecEdgeTiles edges,
                                                          RunBoundsOut rb) {
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ uint64_t sh[kDecThreads / 64];
    load_starts(gp, S);
    __syncthreads();
    const int64_t tile = edges.n > 0 ? edges.t[blockIdx.x] : dec_tile_of_block(S, gp->G, blockIdx.x);
    if (tile < 0) return;  // workgroup-uniform
    if constexpr (MODE == 1) {
        const int64_t tf = tile * kSpTile, tl = std::min<int64_t>(n, tf + kSpTile) - 1;
        if (group_of_elem(S, tf) != group_of_elem(S, tl)) return;  // an edge tile: the MODE 0 launch
    }
    const int t = threadIdx.x;
    const int64_t i0 = tile * kSpTile + t * 4;
    uint32_t d[4];
    if (i0 + 4 <= n) {
        if constexpr (NT) {
            const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(delta + i0));
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(delta + i0);
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = i0 + j < n ? delta[i0 + j] : 0u;
    }
    dec_keys_tile<TN, MODE, NT>(n, gp, gpre, table, tnar, gkeys, gbins, nq, gbn, bn_width, err, S, sh, tile, d,
                                tile_base[tile], (int)threadIdx.x, rb);
}

#ifdef SKML_AB  // A/B form, measured slower (profiles/ab/r05_decp.txt)
// MODE 1 over every inner tile with persistent workgroups: workgroup b walks the tiles that
// dec_tile_of_block deals to its XCD slot (b % 8), and loads the next tile's deltas and base
// while it hashes, gathers and stores the current one.  Same output as k_dec_keys<TN, 1, NT>.
template <typename TN, bool NT>
__global__ __launch_bounds__(kDecThreads) void k_dec_keys_p(const uint32_t* __restrict__ delta, int64_t n,
                                                            const SpGroups* __restrict__ gp,
                                                            const uint64_t* __restrict__ tile_base,
                                                            const uint64_t* __restrict__ gpre,
                                                            const int32_t* __restrict__ table,
                                                            const TN* __restrict__ tnar, int32_t* __restrict__ gkeys,
                                                            int32_t* __restrict__ gbins, int nq, void* __restrict__ gbn,
                                                            int bn_width, unsigned* __restrict__ err, int64_t per_slot,
                                                            RunBoundsOut rb) {
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ uint64_t sh[2][kDecThreads / 64];
    load_starts(gp, S);
    __syncthreads();
    const int64_t slot = blockIdx.x & 7, stride = gridDim.x >> 3;  // gridDim.x: a multiple of 8
    // the j-th tile of this XCD slot's list (-1: past it); edge tiles are skipped (the MODE 0 launch)
    auto tile_at = [&](int64_t j) -> int64_t {
        while (j < per_slot) {
            const int64_t tt = dec_tile_of_block(S, gp->G, j * 8 + slot);
            if (tt < 0) return -1;
            const int64_t tf = tt * kSpTile, tl = std::min<int64_t>(n, tf + kSpTile) - 1;
            if (group_of_elem(S, tf) == group_of_elem(S, tl)) return tt;
            j += stride;  // an edge tile: the next one of this workgroup's walk
        }
        return -1;
    };
    auto load = [&](int64_t tt, uint32_t (&d)[4], uint64_t& tb) {
        const int64_t i0 = tt * kSpTile + threadIdx.x * 4;
        if (i0 + 4 <= n) {
            const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(delta + i0));
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) d[j] = i0 + j < n ? delta[i0 + j] : 0u;
        }
        tb = tile_base[tt];
    };
    int64_t j = blockIdx.x >> 3;
    int64_t tile = tile_at(j);
    uint32_t d[4] = {0, 0, 0, 0}, dn[4] = {0, 0, 0, 0};
    uint64_t tb = 0, tbn = 0;
    if (tile >= 0) load(tile, d, tb);
    int par = 0;
    while (tile >= 0) {
        j += stride;
        const int64_t next = tile_at(j);
        if (next >= 0) load(next, dn, tbn);  // in flight while this tile is decoded
        int tid = threadIdx.x;  // thread-derived values rematerialised per tile (hoisted, they cost registers)
        asm volatile("" : "+v"(tid));
        dec_keys_tile<TN, 1, NT>(n, gp, gpre, table, tnar, gkeys, gbins, nq, gbn, bn_width, err, S, sh[par], tile, d,
                                 tb, tid, rb);
        // (dec_keys_tile returns early past n, after its barrier; every thread of the workgroup
        // still runs the same iterations)
        tile = next;
        par ^= 1;
#pragma unroll
        for (int q = 0; q < 4; q++) d[q] = dn[q];
        tb = tbn;
    }
}
#endif  // SKML_AB


hipError_t launch_dec_keys(hipStream_t st, const uint32_t* delta, int64_t n, const SpGroups* gp, const SpGroups& gh,
                           const uint64_t* tile_base, const uint64_t* gpre, const int32_t* table, const void* tnar,
                           int width, int32_t* gkeys, int32_t* gbins, int nq, void* gbn, int bn_width,
                           unsigned* err, RunBoundsOut rb) {
    if (sp_tiles(n, kSpTile) <= 0) return hipSuccess;
    int64_t per[8] = {};  // tiles per XCD slot (dec_tile_of_block)
    for (int g = 0; g < gh.G; g++) {
        const int64_t t0 = sp_tiles(gh.gstart[g], kSpTile), t1 = sp_tiles(gh.gstart[g + 1], kSpTile);
        if (t1 > t0) per[g & 7] += t1 - t0;
    }
    int64_t most = 0;
    for (int x = 0; x < 8; x++) most = std::max(most, per[x]);
    const unsigned grid = (unsigned)(8 * most);
    // MODE 1 over every tile, then MODE 0 over the edge tiles; MODE 0 alone for other shapes, for
    // tables past 2^31 cells (MODE 1's cells are 32-bit offsets and its modulus takes cols <=
    // 2^30), and under SKML_FORM_DEC_ROWS_SERIAL (tests)
    const bool batched = gh.rows == 2 && (table != nullptr || (tnar != nullptr && width < 32)) &&
                         form(SKML_FORM_DEC_ROWS_SERIAL) != 1 &&
                         gh.ncells <= ((int64_t)1 << 31);
    DecEdgeTiles all{}, edges{};
    all.n = 0;
    if (batched) {  // tiles holding a group edge that is not a tile edge
        for (int g = 1; g < gh.G; g++) {
            const int64_t e = gh.gstart[g];
            if (e <= 0 || e >= n || e % kSpTile == 0 || gh.gstart[g + 1] == e) continue;
            const int64_t t = e / kSpTile;
            if (edges.n == 0 || edges.t[edges.n - 1] != t) edges.t[edges.n++] = t;
        }
    }
    // nontemporal streams (decode 0.73 -> 0.71 ms, profiles/ab/r04_sparse_restore_aggregate.txt)
#define SKML_DEC_LAUNCH(TNT, MODE, GRID, TILES, TNPTR)                                                            \
    hipLaunchKernelGGL((k_dec_keys<TNT, MODE>), dim3(GRID), dim3(kDecThreads), 0, st, delta, n, gp, tile_base, gpre, \
                       table, TNPTR, gkeys, gbins, nq, gbn, bn_width, err, TILES, rb)
    // MODE 1 with one workgroup per tile; SKML_FORM_DEC_ROWS_SERIAL = 2 selects persistent
    // workgroups with the next tile's deltas in flight (measured slower at 2^28: restore 0.767
    // vs 0.707 ms, profiles/ab/r05_decp.txt; kept as an A/B form)
#ifdef SKML_AB
    const bool persistent = form(SKML_FORM_DEC_ROWS_SERIAL) == 2;
#define SKML_DEC_PERSISTENT(TNT, TNPTR)                                                          \
        if (batched && persistent) {                                                      \
            static const int res = resident_blocks(k_dec_keys_p<TNT, true>, kDecThreads); \
            const int64_t ps = res > 0 ? std::max<int64_t>(1, std::min<int64_t>(most, res / 8)) : most; \
            hipLaunchKernelGGL((k_dec_keys_p<TNT, true>), dim3((unsigned)(8 * ps)), dim3(kDecThreads), 0, st, delta, \
                               n, gp, tile_base, gpre, table, TNPTR, gkeys, gbins, nq, gbn, bn_width, err, most, rb); \
            if (edges.n > 0) SKML_DEC_LAUNCH(TNT, 0, (unsigned)edges.n, edges, TNPTR);    \
        } else
#else
#define SKML_DEC_PERSISTENT(TNT, TNPTR)
#endif
#define SKML_DEC_WIDTH(TNT, TNPTR)                                                          \
    do {                                                                                  \
        SKML_DEC_PERSISTENT(TNT, TNPTR)                                                   \
        if (batched) {                                                                    \
            hipLaunchKernelGGL((k_dec_keys<TNT, 1, true>), dim3(grid), dim3(kDecThreads), 0, st, delta, n, gp,    \
                               tile_base, gpre, table, TNPTR, gkeys, gbins, nq, gbn, bn_width, err, all, rb); \
            if (edges.n > 0) SKML_DEC_LAUNCH(TNT, 0, (unsigned)edges.n, edges, TNPTR);    \
        } else {                                                                          \
            SKML_DEC_LAUNCH(TNT, 0, grid, all, TNPTR);                                    \
        }                                                                                 \
    } while (0)
    if (width == 8) SKML_DEC_WIDTH(uint8_t, static_cast<const uint8_t*>(tnar));
    else if (width == 16) SKML_DEC_WIDTH(uint16_t, static_cast<const uint16_t*>(tnar));
    else SKML_DEC_WIDTH(int32_t, static_cast<const int32_t*>(nullptr));
#undef SKML_DEC_WIDTH
#undef SKML_DEC_PERSISTENT
#undef SKML_DEC_LAUNCH
    return hipGetLastError();
}

}  // namespace skml
