// skml_sparse.hip -- CDNA4 (gfx950) kernels of the sparse codec: Gradient.sum and Sort.merge over
// restored payloads.
//   k_agg_*          Gradient.sum of restored payloads, tiled over the dense sum.
//   k_merge_round    Sort.merge (util/Sort.java:362-379) as rounds of stable merge-path merges.
//   k_rs_*           Sort.merge in one pass over key ranges (the regular case).
// The other stages have files of their own: skml_sparse_compact / _partition / _minmax / _delta /
// _huffman.hip.  The sum and the merge share this translation unit.  The optimiser propagates a
// helper's argument ranges from all the callers it sees: with the sum alone, agg_search32's n is
// the constant 65 and k_agg_tiles_w compiles to other code than beside k_rs_merge.
#include <algorithm>
#include <type_traits>

#include "skml_device.hpp"
#include "skml_sparse.h"
#include "skml_sparse_device.hpp"

namespace skml {

// ---- Gradient.sum of P restored payloads, tiled over the dense sum (skml_sparse_decode_sum_f64) ----
// Each payload is restored (DeltaAdaptive keys + MinMax bins, grouped order, no Sort.merge) into
// scratch; k_agg_bounds records where every (payload, group) run enters each dense tile of
// kAggTile keys; k_agg_tiles then builds each tile of the double sum in LDS, payload after payload
// in payload order (keys are unique within a payload: no atomics), and writes it once.  The dense
// sum is read and written once instead of one random read-modify-write per restored key.
// bounds[g * (ntiles + 1) + t] = first element (payload index) of group g's run with key >=
// t * kAggTile; 0 throughout for an empty group.
#ifdef SKML_AB  // the runs' bounds in passes of their own (SKML_FORM_RUN_BOUNDS = 1); the key query writes them
// Run bounds over 16 consecutive restored keys per thread (four 16-byte loads and the key before
// them; the group's ends in registers): for each element, the ranges between its predecessor's
// range and its own get the element's index, and a run's last element closes its run.
// AGG: Gradient.sum's tiles of kAggTile keys (clamped to ntiles, tail filled to ntiles, keys
// checked against [0, dim)); else Sort.merge's ranges of kRsRange keys (last range + 1 and the
// range maxima into info, INT32_MAX and negative keys flagged irregular).  Both flag a key that
// does not ascend inside its run.
template <bool AGG>
__device__ __forceinline__ void run_bounds16(const int32_t* __restrict__ gk, int64_t n, const int64_t* S,
                                             int32_t* __restrict__ bounds, int64_t ld, int64_t ntiles, int64_t dim,
                                             RsInfo* __restrict__ info, unsigned& bad, int tile_bits = 12) {
    constexpr int kPer = 16;
    const int64_t i0 = ((int64_t)blockIdx.x * kSpThreads + threadIdx.x) * kPer;
    if (i0 >= n) return;
    int32_t key[kPer];
    if (i0 + kPer <= n && (reinterpret_cast<uintptr_t>(gk) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < kPer / 4; q++) {
            const int4 v = *reinterpret_cast<const int4*>(gk + i0 + 4 * q);
            key[4 * q] = v.x, key[4 * q + 1] = v.y, key[4 * q + 2] = v.z, key[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < kPer; e++) key[e] = i0 + e < n ? gk[i0 + e] : 0;
    }
    int32_t prev = i0 > 0 ? gk[i0 - 1] : 0;
    int g = group_of_elem(S, i0);
    int64_t lo = S[g], hi = S[g + 1];
    auto tile_of = [&](int32_t k) -> int64_t {
        if constexpr (AGG) return k < 0 ? 0 : std::min<int64_t>((int64_t)(k >> tile_bits), ntiles);
        else return (int64_t)(k >> kRsBits);
    };
#pragma unroll
    for (int e = 0; e < kPer; e++) {
        const int64_t i = i0 + e;
        if (i >= n) break;
        while (i >= hi) {  // the next non-empty run (rare: at most G - 1 times over all threads)
            g++;
            lo = S[g];
            hi = S[g + 1];
        }
        const int32_t k = key[e];
        const bool first = i == lo;
        bool ok;
        if constexpr (AGG) {
            if (k < 0 || (int64_t)k >= dim) bad = 1;  // SparseDoubleGradient's bound check
            // keys ascend strictly inside a group (the tiles add without atomics)
            if (!first && k <= prev) bad = 1;
            ok = true;
        } else {
            ok = !(k < 0 || k == INT32_MAX || (!first && k <= prev));
            if (!ok) bad = 1;
        }
        if (ok) {
            const int64_t ti = tile_of(k);
            const int64_t pt = first || (!AGG && prev < 0) ? -1 : tile_of(prev);
            int32_t* b = bounds + (int64_t)g * ld;
            for (int64_t t = pt + 1; t <= ti; t++) b[t] = (int32_t)i;
            if (i == hi - 1) {
                if constexpr (AGG) {
                    for (int64_t t = ti + 1; t <= ntiles; t++) b[t] = (int32_t)hi;
                } else {  // the run's last range ends at the run's end
                    b[ti + 1] = (int32_t)hi;
                    info->tlast1[g] = (int32_t)ti + 1;
                    atomicMax(&info->tmax1, (int32_t)ti + 1);
                }
            }
        }
        prev = k;
    }
}

__global__ __launch_bounds__(kSpThreads) void k_agg_bounds(const int32_t* __restrict__ gk, int64_t n,
                                                           const SpGroups* __restrict__ gp, int64_t ntiles, int64_t dim,
                                                           int32_t* __restrict__ bounds, unsigned* __restrict__ err,
                                                           int tile_bits) {
    __shared__ int64_t S[kMaxGroups + 1];
    load_starts(gp, S);
    __syncthreads();
    unsigned bad = 0;
    run_bounds16<true>(gk, n, S, bounds, ntiles + 1, ntiles, dim, nullptr, bad, tile_bits);
    if (bad) atomicOr(err, 1u);
}
hipError_t launch_agg_bounds(hipStream_t st, const int32_t* gk, int64_t n, const SpGroups* gp, int64_t ntiles,
                             int64_t dim, int32_t* bounds, unsigned* err, int tile_bits) {
    if (n <= 0) return hipSuccess;
    const int64_t grid = sp_tiles(sp_tiles(n, 16), kSpThreads);  // 16 keys per thread
    hipLaunchKernelGGL(k_agg_bounds, dim3((unsigned)grid), dim3(kSpThreads), 0, st, gk, n, gp, ntiles, dim, bounds, err,
                       tile_bits);
    return hipGetLastError();
}
#endif  // SKML_AB

// Loads through AggPayload's pointers as global (address space 1) loads.  The pointers come from
// memory (the payload table, copied to LDS or registers), so the compiler would emit flat loads,
// which count on lgkmcnt as well: every later LDS wait would then wait for them too, one memory
// round trip per element batch instead of one per tile.
template <typename T>
__device__ __forceinline__ T gload(const void* p, int64_t i) {
    return ((const __attribute__((address_space(1))) T*)p)[i];
}
constexpr int kAggPB = 8, kAggThreads = 512, kAggLdsValues = 256;
static_assert(kAggPB == kAggVPayloads, "eight payloads per batch in both tile forms");
__device__ __forceinline__ int agg_search32(const int32_t* pre, int n, int j) {  // largest i < n: pre[i] <= j
    int i = 0;
    for (int step = 32; step >= 1; step >>= 1)
        if (i + step < n && pre[i + step] <= j) i += step;
    return i;
}

// Gradient.sum over tiles of kAggTile keys, one wave per payload of a batch (8 waves, 8
// payloads): the wave walks its payload's group runs in this tile (run bounds from k_agg_bounds),
// one lane per element; every wave loads its elements' keys and bins first, then the waves add
// into the LDS tile one after the other in payload order (one barrier per payload).  Up to
// kAggWPer elements per lane are held in registers, a longer payload (a dense form, or a tile far
// denser than the mean) adds the rest in further rounds of its turn.  Each wave marks its
// payload's keys in a presence bitmap of the tile as it adds them (an LDS atomic OR with return):
// a bit already set is a key repeated across the payload's groups, which the reference's
// SparseDoubleGradient constructor rejects (err bit 2).  The general form: any P, G and nq.
constexpr int kAggWPer = 8;
// A persistent grid walks the tiles strided: unit u = b * units-per-workgroup + sub takes tiles
// u, u + units, ..., so all units sweep the sum together (one write front).  Measured and dropped
// (round 4, profiles/ab/r04_sparse_aggregate_tiles.txt): an XCD-aware renumbering (equal: 1,826
// against 1,822 us) and a contiguous share per unit (5.87-5.92 -> 6.60-6.62 ms end to end: 4,096
// separate write fronts).
struct TileWalk {
    int64_t t0, t1, step;
};
__device__ __forceinline__ TileWalk tile_walk(int64_t blk, int64_t nblk, int sub, int nsub, int64_t ntiles) {
    return {blk * nsub + sub, ntiles, nblk * nsub};
}
// The same sweep with each round's tiles dealt to the XCDs in contiguous segments: workgroup b runs
// on XCD b % 8, so within a round XCD x takes tiles [x, x + 1) * (nblk / 8) * nsub and its
// workgroups take consecutive nsub-tile groups of that segment.  Neighbouring tiles share the
// cache lines of the payloads' run pieces (a 128-byte line of keys spans ~5 tiles of a C3 piece,
// of bins ~20): dealt round-robin, each line was fetched into several XCDs' L2 (the sum-tile kernel
// read 3.96 GB per 1.1 GB of elements, profiles/r05m_agg_pmc.json).  One write front per XCD.
__device__ __forceinline__ TileWalk tile_walk_xcd(int64_t blk, int64_t nblk, int sub, int nsub, int64_t ntiles) {
    if (nblk % 8 != 0) return tile_walk(blk, nblk, sub, nsub, ntiles);
    return {(blk % 8) * (nblk / 8) * nsub + (blk / 8) * nsub + sub, ntiles, nblk * nsub};
}
// Output types of the sum (skml_sparse_decode_sum_f64 / _f32 / _bf16 / _f16).  The sum itself is
// always double; a narrow type appears only in the store of a finished tile: the double, x scale,
// rounded to float and (bf16 / fp16) rounded again, the dense decode-sum's definition, with
// skml_device.hpp's conversions.  A launch that continues a sum (from_out) reads the doubles of
// `src`: `out` itself for double, else the accumulator the earlier launches wrote.
// kAggOutVec: values of one 16-byte store.
template <typename O>
constexpr int agg_out_vec() { return 16 / (int)sizeof(O); }
// v[0..kV) (sums, x scale applied) to out[x..x + kV), out + x 16-byte aligned
template <typename O, int kV = agg_out_vec<O>()>
__device__ __forceinline__ void agg_store_vec(O* out, int64_t x, const double (&v)[kV]) {
    static_assert(!std::is_same<O, double>::value, "the double tiles store their double2 themselves");
    if constexpr (std::is_same<O, float>::value) {
        typedef float f32x4_v __attribute__((ext_vector_type(4)));
        const f32x4_v o = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        *reinterpret_cast<f32x4_v*>(out + x) = o;
    } else {
        const u32x4_v o = {narrow2<O>((float)v[0], (float)v[1]), narrow2<O>((float)v[2], (float)v[3]),
                           narrow2<O>((float)v[4], (float)v[5]), narrow2<O>((float)v[6], (float)v[7])};
        *reinterpret_cast<u32x4_v*>(out + x) = o;
    }
}

template <typename O>
__device__ __forceinline__ void agg_tiles_w_body(const AggPayload* __restrict__ pays, int P, int64_t ntiles,
                                                 int64_t dim, O* out, const double* src, int from_out, double scale,
                                                 unsigned* __restrict__ err) {
    static_assert(kAggThreads / 64 == kAggPB, "one wave per payload of a batch");
    __shared__ double acc[kAggTile];
    __shared__ uint32_t here[kAggPB][kAggTile / 32];  // presence bits, one bitmap per wave
    __shared__ double qt[kAggPB][kAggLdsValues];
    __shared__ int32_t rb[kAggPB][kMaxGroups + 1];  // run prefix (elements) per group, this tile
    __shared__ int32_t rs[kAggPB][kMaxGroups];      // run start (element index in the payload)
    __shared__ int32_t dfs[kAggPB];                 // dense_form of the batch's payloads
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // a persistent grid: with one batch (P <= kAggPB) the payloads and their quantValues are read
    // once per workgroup instead of once per tile
    const bool one_batch = P <= kAggPB;
    AggPayload a{};
    auto load_batch = [&](int p0, int np) {
        if (wave < np) {
            a = pays[p0 + wave];
            for (int b = lane; b < kAggLdsValues; b += 64)
                if (a.nq <= kAggLdsValues && b < a.nq) qt[wave][b] = gload<double>(a.qv, b);
            if (lane == 0) dfs[wave] = a.dense_form;
        }
    };
    if (one_batch) load_batch(0, P);
    // with one batch, lane g of wave p holds the next tile's run bounds of payload p, group g:
    // loaded one tile ahead, so a tile's element loads wait on one memory round trip, not two
    int32_t nb0 = 0, nb1 = 0;
    auto fetch_bounds = [&](int64_t tt) {
        if (one_batch && wave < P && lane < a.G && tt < ntiles) {
            const int32_t* bd = a.bounds + (int64_t)lane * (ntiles + 1);
            nb0 = gload<int32_t>(bd, tt);
            nb1 = gload<int32_t>(bd, tt + 1);
        }
    };
    const TileWalk tw = tile_walk(blockIdx.x, gridDim.x, 0, 1, ntiles);
    fetch_bounds(tw.t0);
    unsigned bad = 0;
    // The store of tile t - 1 is deferred until tile t's element loads are in flight, and the
    // zeroing of the LDS sum follows it, so both overlap those loads' latency.
    int64_t prev_k0 = -1, prev_nk = 0;
    auto store_prev = [&]() {
        if constexpr (std::is_same<O, double>::value) {
            if (prev_k0 >= 0)
                for (int x = threadIdx.x; x < prev_nk; x += kAggThreads)
                    out[prev_k0 + x] = scale == 1.0 ? acc[x] : __dmul_rn(acc[x], scale);
        } else {
            if (prev_k0 < 0) return;
            constexpr int kV = agg_out_vec<O>();
            O* o = out + prev_k0;
            static_assert(kAggTile % (kV * kAggThreads) == 0, "whole rounds of 16-byte stores");
            if (prev_nk == kAggTile && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {  // 16 B per lane
                for (int x = kV * threadIdx.x; x < kAggTile; x += kV * kAggThreads) {
                    double v[kV];
#pragma unroll
                    for (int i = 0; i < kV; i++) v[i] = scale == 1.0 ? acc[x + i] : __dmul_rn(acc[x + i], scale);
                    agg_store_vec<O>(o, x, v);
                }
            } else {
                for (int x = threadIdx.x; x < prev_nk; x += kAggThreads)
                    store_narrow<O>(o, x, (float)(scale == 1.0 ? acc[x] : __dmul_rn(acc[x], scale)));
            }
        }
    };
    for (int64_t t = tw.t0; t < tw.t1; t += tw.step) {
        const int64_t k0 = t * kAggTile, nk = std::min<int64_t>(kAggTile, dim - k0);
        const int32_t cb0 = nb0, cb1 = nb1;  // this tile's bounds (one batch)
        fetch_bounds(t + tw.step);
        for (int p0 = 0; p0 < P; p0 += kAggPB) {
            const int np = std::min(kAggPB, P - p0);
            __syncthreads();  // the previous batch / tile is done with qt / rb / rs / acc's adds
            if (!one_batch) load_batch(p0, np);
            const bool mine = wave < np;
            if (mine) {
                int32_t len = 0;
                if (lane < a.G) {
                    int32_t b0 = cb0, b1 = cb1;
                    if (!one_batch) {
                        const int32_t* bd = a.bounds + (int64_t)lane * (ntiles + 1);
                        b0 = gload<int32_t>(bd, t);
                        b1 = gload<int32_t>(bd, t + 1);
                    }
                    len = b1 > b0 ? b1 - b0 : 0;
                    rs[wave][lane] = b0;
                }
                int32_t x = len;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int32_t y = __shfl_up(x, off, 64);
                    if (lane >= off) x += y;
                }
                if (lane < kMaxGroups) rb[wave][lane + 1] = x;
                if (lane == 0) rb[wave][0] = 0;
                reinterpret_cast<uint64_t*>(here[wave])[lane] = 0;  // 128 words: two per lane
            }
            __syncthreads();
            // this wave's elements: compact index j = lane + 64 u over the concatenated runs; the run
            // holding j by a walk over the (few) run prefixes
            const int total = mine ? rb[wave][a.G] : 0;
            const bool lds_q = a.nq <= kAggLdsValues;
            // the run holding j: with at most 8 groups, a count of the run ends (held in registers)
            // at or below j; else a binary search of the 65 prefix entries
            int32_t re[8];
#pragma unroll
            for (int q = 0; q < 8; q++) re[q] = rb[wave][q + 1];
            const bool few_g = a.G <= 8;
            auto run_of = [&](int j) -> int {
                if (few_g) {
                    int g = 0;
#pragma unroll
                    for (int q = 0; q < 8; q++) g += re[q] <= j ? 1 : 0;
                    return g;
                }
                return agg_search32(rb[wave], kMaxGroups + 1, j);
            };
            int32_t kk[kAggWPer];
            double vv[kAggWPer];
#pragma unroll
            for (int u = 0; u < kAggWPer; u++) {
                const int j = lane + 64 * u;
                kk[u] = 0;
                vv[u] = 0.0;
                if (j < total) {
                    const int g = run_of(j);
                    const int64_t i = (int64_t)rs[wave][g] + (j - rb[wave][g]);
                    kk[u] = gload<int32_t>(a.gk, i);
                    const uint32_t b = a.bw == 1 ? gload<uint8_t>(a.gb, i) : gload<uint16_t>(a.gb, i);
                    vv[u] = lds_q ? qt[wave][b] : gload<double>(a.qv, b);
                }
            }
            if (p0 == 0) {  // the previous tile leaves, this tile's sum starts (loads in flight)
                store_prev();
                __syncthreads();
                for (int x = threadIdx.x; x < kAggTile; x += kAggThreads)
                    acc[x] = (from_out && x < nk) ? src[k0 + x] : 0.0;
                __syncthreads();
                prev_k0 = k0;
                prev_nk = nk;
            }
            for (int pl = 0; pl < np; pl++) {
                if (wave == pl) {
                    const bool dform = a.dense_form != 0;
                    // a key outside this tile is an error (k_agg_bounds placed it here), and so is a
                    // key already marked in this payload's bitmap: then two lanes of one instruction
                    // may have added it racily, but the sum is refused anyway.  The dense form keeps
                    // |v| > EPS only (SparseDoubleGradient.toDense).
#define SKML_AGG_ADD(K, V)                                                        \
    do {                                                                          \
        const int32_t k_ = (K);                                                   \
        const double v_ = (V);                                                    \
        if (k_ < k0 || (int64_t)k_ >= k0 + nk) {                                  \
            bad |= 1u;                                                            \
        } else {                                                                  \
            const int x_ = (int)(k_ - k0);                                        \
            const uint32_t bit_ = 1u << (x_ & 31);                                \
            if (atomicOr(&here[wave][x_ >> 5], bit_) & bit_) bad |= 2u;           \
            if (!dform || fabs(v_) > 1e-8) acc[x_] += v_;                         \
        }                                                                         \
    } while (0)
#pragma unroll
                    for (int u = 0; u < kAggWPer; u++)
                        if (lane + 64 * u < total) SKML_AGG_ADD(kk[u], vv[u]);
                    for (int j = lane + 64 * kAggWPer; j < total; j += 64) {  // the rest of a long payload
                        const int g = run_of(j);
                        const int64_t i = (int64_t)rs[wave][g] + (j - rb[wave][g]);
                        const uint32_t b = a.bw == 1 ? gload<uint8_t>(a.gb, i) : gload<uint16_t>(a.gb, i);
                        SKML_AGG_ADD(gload<int32_t>(a.gk, i), lds_q ? qt[wave][b] : gload<double>(a.qv, b));
                    }
#undef SKML_AGG_ADD
                }
                __syncthreads();
                if (dfs[pl]) {  // the dense form adds +0.0 elsewhere: -0.0 sums become +0.0
                    for (int x = threadIdx.x; x < kAggTile; x += kAggThreads)
                        if (__double_as_longlong(acc[x]) == (long long)0x8000000000000000ull) acc[x] = 0.0;
                    __syncthreads();
                }
            }
        }
    }
    __syncthreads();
    store_prev();
    if (bad) atomicOr(err, bad);
}
__global__ __launch_bounds__(kAggThreads) void k_agg_tiles_w(const AggPayload* __restrict__ pays, int P,
                                                            int64_t ntiles, int64_t dim, double* __restrict__ out,
                                                            int from_out, double scale, unsigned* __restrict__ err) {
    agg_tiles_w_body<double>(pays, P, ntiles, dim, out, out, from_out, scale, err);
}
// the same sum stored as float / bf16 / fp16, continued from the double accumulator `src`
template <typename O>
__global__ __launch_bounds__(kAggThreads) void k_agg_tiles_w_o(const AggPayload* __restrict__ pays, int P,
                                                              int64_t ntiles, int64_t dim, O* __restrict__ out,
                                                              const double* __restrict__ src, int from_out,
                                                              double scale, unsigned* __restrict__ err) {
    agg_tiles_w_body<O>(pays, P, ntiles, dim, out, src, from_out, scale, err);
}

// One wave per tile of kAggVTile keys, staged: lane 8p + g of the wave holds the run piece of
// payload p, group g (P <= 8, G <= 8), the pieces are concatenated payload by payload and each lane
// loads up to kAggWPer * SUB elements of the concatenation.  The wave then writes every element's
// bin to its slot of the wave's stage (one byte per (payload, key)) and sets the slot's presence
// bit; a bit already set is a key repeated inside one payload (err bit 2).  Last, lane l owns keys
// 8l .. 8l + 7 and sums them in registers payload after payload, which is Gradient.sum's order for
// every key, without a read-modify-write of an LDS sum per element.  Persistent waves: each wave
// loads its next tile's run bounds one tile ahead, and stores a tile's sums after the next tile's
// element loads are in flight.  bw == 1 and nq <= 256 for every payload (agg_vtiles_ok).
// SUB > 1: a wave takes SUB consecutive tiles at once (one bounds pair and one round of element
// loads for all of them: run pieces SUB times longer, so fewer L2 requests per element), then
// stages and sums them one tile after the other through the same 4 KB stage.
constexpr int kAggVBits = 9, kAggVTile = 1 << kAggVBits;
static_assert(kAggVTile == 8 * 64, "eight keys per lane");
#ifdef SKML_AB  // A/B forms of the sum tile (SKML_FORM_AGG_TILES 2..5), measured slower than k_agg_rmw
template <int SUB>
__global__ __launch_bounds__(kAggThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_agg_vtiles(
    const AggPayload* __restrict__ pays, int P, int64_t ntiles, int64_t dim, double* __restrict__ out, int from_out,
    double scale, unsigned* __restrict__ err, const int32_t* __restrict__ kbase, const uint8_t* __restrict__ bbase) {
    constexpr int kWaves = kAggThreads / 64;
    constexpr int kPer = kAggWPer * SUB;  // elements per lane held in registers
    // the stage: a bin per (payload, key); between tiles, the transpose of the stored sums
    __shared__ __attribute__((aligned(16))) uint8_t bins[kWaves][kAggPB][kAggVTile];
    static_assert(kAggPB * kAggVTile == kAggVTile * sizeof(double), "a tile of sums fits the stage");
    __shared__ uint32_t here[kWaves][kAggPB][kAggVTile / 32];  // presence bits
    __shared__ double qt[kAggPB][kAggLdsValues];
    __shared__ int32_t pre[kWaves][65];  // the wave's 64 run pieces, scanned
    __shared__ int32_t pk0[kWaves][64];  // each piece's first key (index from kbase)
    __shared__ int32_t pn0[kWaves][64];  // and its first bin (byte from bbase)
    __shared__ AggPayload pl[kAggPB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < P * (int)(sizeof(AggPayload) / 8))
        reinterpret_cast<uint64_t*>(pl)[threadIdx.x] = reinterpret_cast<const uint64_t*>(pays)[threadIdx.x];
    __syncthreads();
    if (wave < P)
        for (int b = lane; b < pl[wave].nq; b += 64) qt[wave][b] = gload<double>(pl[wave].qv, b);
    __syncthreads();
    const int pl_l = lane >> 3, g_l = lane & 7;
    const bool lane_on = pl_l < P && g_l < pl[pl_l].G;
    const int32_t* bd = lane_on ? pl[pl_l].bounds + (int64_t)g_l * (ntiles + 1) : nullptr;
    uint8_t(*B)[kAggVTile] = bins[wave];
    uint32_t(*H)[kAggVTile / 32] = here[wave];
    unsigned bad = 0;
    const int64_t nsup = (ntiles + SUB - 1) / SUB;  // super-tiles of SUB tiles
    int32_t nb0 = 0, nb1 = 0;
    auto fetch = [&](int64_t tt) {
        if (lane_on && tt < nsup) {
            nb0 = gload<int32_t>(bd, tt * SUB);
            nb1 = gload<int32_t>(bd, std::min<int64_t>(tt * SUB + SUB, ntiles));
        }
    };
    int64_t prev_k0 = -1, prev_nk = 0;
    // a tile's sums (lane l: keys 8l .. 8l + 7) wait in the stage until the next loads are in
    // flight (the last tile of a super-tile) or the next tile is staged, and leave transposed, so
    // each 16-byte store instruction covers 1 KB of the sum
    double* T = reinterpret_cast<double*>(&B[0][0]);
    auto store_prev = [&](int l) {
        if (prev_k0 < 0) return;
        double* o = out + prev_k0;
        const bool whole = prev_nk == kAggVTile && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int x = 128 * q + 2 * l;
            const double2 v = *reinterpret_cast<const double2*>(T + x);
            if (whole) {
                *reinterpret_cast<double2*>(o + x) = v;
            } else {
                if (x < prev_nk) o[x] = v.x;
                if (x + 1 < prev_nk) o[x + 1] = v.y;
            }
        }
        __builtin_amdgcn_wave_barrier();
        prev_k0 = -1;
    };
    const TileWalk tw = tile_walk(blockIdx.x, gridDim.x, wave, kWaves, nsup);
    fetch(tw.t0);
    for (int64_t t = tw.t0; t < tw.t1; t += tw.step) {
        // lane-derived values are recomputed each tile behind an empty asm barrier: hoisted out of
        // the loop (32 element indices, shuffle addresses) they were spilled to scratch
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int64_t K0 = t * SUB << kAggVBits, NK = std::min<int64_t>((int64_t)SUB << kAggVBits, dim - K0);
        const int32_t b0 = nb0, b1 = nb1;
        fetch(t + tw.step);
        const int32_t len = lane_on && b1 > b0 ? b1 - b0 : 0;
        const int32_t x = (int32_t)wave_incl_scan_u32((uint32_t)len);  // DPP scan: no lane-id addresses
        pre[wave][ln + 1] = x;
        if (ln == 0) pre[wave][0] = 0;
        pk0[wave][ln] = lane_on ? pl[pl_l].gk_off + b0 : 0;
        pn0[wave][ln] = lane_on ? pl[pl_l].gb_off + b0 : 0;
        const int total = __builtin_amdgcn_readlane(x, 63);
        __builtin_amdgcn_wave_barrier();
        auto piece_of = [&](int j) -> int {  // largest s < 64 with pre[s] <= j
            int s_ = 0;
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1)
                if (pre[wave][s_ + step] <= j) s_ += step;
            return s_;
        };
        // eight elements' pieces first (independent LDS searches), then their loads
        int32_t kk[kPer];
        uint32_t bb[kPer];
#pragma unroll
        for (int u0 = 0; u0 < kPer; u0 += kAggWPer) {
            int spc[kAggWPer];
#pragma unroll
            for (int u = 0; u < kAggWPer; u++) {
                const int j = ln + 64 * (u0 + u);
                spc[u] = piece_of(j < total ? j : 0);
            }
#pragma unroll
            for (int u = 0; u < kAggWPer; u++) {
                const int j = ln + 64 * (u0 + u);
                kk[u0 + u] = INT32_MIN;
                bb[u0 + u] = 0;
                if (j < total) {
                    const int sp = spc[u], p = sp >> 3, d = j - pre[wave][sp];
                    kk[u0 + u] = gload<int32_t>(kbase, (uint32_t)(pk0[wave][sp] + d));
                    bb[u0 + u] = gload<uint8_t>(bbase, (uint32_t)(pn0[wave][sp] + d)) | ((uint32_t)p << 8);
                }
            }
        }
        // one word per element: key offset in the super-tile (bits 0..12), bin (13..20), payload
        // (21..23); ~0u: no element.  A key outside the super-tile is an error (k_agg_bounds placed
        // it here).
        uint32_t ew[kPer];
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int64_t off = (int64_t)kk[u] - K0;
            ew[u] = ~0u;
            if (ln + 64 * u < total) {
                if (off < 0 || off >= NK) bad |= 1u;
                else ew[u] = (uint32_t)off | ((bb[u] & 0xFFu) << 13) | ((bb[u] >> 8) << 21);
            }
        }
        store_prev(ln);  // after this super-tile's loads are issued
#pragma unroll 1
        for (int sub = 0; sub < SUB; sub++) {
            const int64_t k0 = K0 + ((int64_t)sub << kAggVBits);
            const int64_t nk = std::min<int64_t>(kAggVTile, dim - k0);
            if (nk <= 0) break;
            int ls = ln;  // (rematerialised per tile, like ln)
            asm volatile("" : "+v"(ls));
            if (sub > 0) store_prev(ls);  // the previous tile's sums leave the stage before it is reused
            reinterpret_cast<uint64_t*>(H)[ls] = 0;  // 8 x 16 words: two per ls
            __builtin_amdgcn_wave_barrier();
            const uint32_t sub_lo = (uint32_t)sub << kAggVBits;
            auto stage = [&](uint32_t w) {  // w: an element word of this tile
                const int p = (int)(w >> 21), xk = (int)((w & 0x1FFFu) - sub_lo);
                B[p][xk] = (uint8_t)(w >> 13);
                const uint32_t bit = 1u << (xk & 31);
                if (atomicOr(&H[p][xk >> 5], bit) & bit) bad |= 2u;  // a key twice in one payload
            };
#pragma unroll
            for (int u = 0; u < kPer; u++)
                if (ew[u] != ~0u && ((ew[u] & 0x1FFFu) >> kAggVBits) == (uint32_t)sub) stage(ew[u]);
            for (int j = 64 * kPer + ls; j < total; j += 64) {  // elements past the registers
                const int sp = piece_of(j), p = sp >> 3, d = j - pre[wave][sp];
                const int64_t off = (int64_t)gload<int32_t>(kbase, (uint32_t)(pk0[wave][sp] + d)) - K0;
                if (off < 0 || off >= NK) {
                    bad |= 1u;
                    continue;
                }
                if ((off >> kAggVBits) == sub)
                    stage((uint32_t)off | ((uint32_t)gload<uint8_t>(bbase, (uint32_t)(pn0[wave][sp] + d)) << 13) |
                          ((uint32_t)p << 21));
            }
            __builtin_amdgcn_wave_barrier();
            // ls l: keys 8l .. 8l + 7, payload after payload
            double acc[8];
#pragma unroll
            for (int i = 0; i < 8; i++)  // a later batch continues the sum
                acc[i] = from_out && 8 * ls + i < nk ? out[k0 + 8 * ls + i] : 0.0;
            for (int p = 0; p < P; p++) {
                const uint32_t m = reinterpret_cast<const uint8_t*>(H[p])[ls];
                const uint2 bw8 = *reinterpret_cast<const uint2*>(&B[p][8 * ls]);
                const bool dform = pl[p].dense_form != 0;
                double v[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const uint32_t b = ((i < 4 ? bw8.x : bw8.y) >> (8 * (i & 3))) & 0xFFu;
                    v[i] = 0.0;
                    if (m & (1u << i)) v[i] = qt[p][b];
                }
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    // the dense form keeps |v| > EPS only (SparseDoubleGradient.toDense), and adds +0.0
                    // elsewhere: a -0.0 sum becomes +0.0
                    if ((m & (1u << i)) && (!dform || fabs(v[i]) > 1e-8)) acc[i] += v[i];
                    if (dform && __double_as_longlong(acc[i]) == (long long)0x8000000000000000ull) acc[i] = 0.0;
                }
            }
            if (scale != 1.0)
#pragma unroll
                for (int i = 0; i < 8; i++) acc[i] = __dmul_rn(acc[i], scale);
            __builtin_amdgcn_wave_barrier();  // the stage is read before the sums replace it
#pragma unroll
            for (int q = 0; q < 4; q++)
                *reinterpret_cast<double2*>(T + 8 * ls + 2 * q) = make_double2(acc[2 * q], acc[2 * q + 1]);
            __builtin_amdgcn_wave_barrier();
            prev_k0 = k0;
            prev_nk = nk;
        }
    }
    store_prev(lane);
    if (bad) atomicOr(err, bad);
}

// The staged tiles with the next tile's element loads in flight while this tile is staged and
// summed (software pipelined: run bounds two tiles ahead, elements one tile ahead, the piece tables
// double-buffered in LDS).  Same sums as k_agg_vtiles<1>.
__global__ __launch_bounds__(kAggThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_agg_vtiles_pf(
    const AggPayload* __restrict__ pays, int P, int64_t ntiles, int64_t dim, double* __restrict__ out, int from_out,
    double scale, unsigned* __restrict__ err, const int32_t* __restrict__ kbase, const uint8_t* __restrict__ bbase) {
    constexpr int kWaves = kAggThreads / 64;
    __shared__ __attribute__((aligned(16))) uint8_t bins[kWaves][kAggPB][kAggVTile];
    __shared__ uint32_t here[kWaves][kAggPB][kAggVTile / 32];
    __shared__ double qt[kAggPB][kAggLdsValues];
    __shared__ int32_t pre[2][kWaves][65];
    __shared__ int32_t pk0[2][kWaves][64];
    __shared__ int32_t pn0[2][kWaves][64];
    __shared__ AggPayload pl[kAggPB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < P * (int)(sizeof(AggPayload) / 8))
        reinterpret_cast<uint64_t*>(pl)[threadIdx.x] = reinterpret_cast<const uint64_t*>(pays)[threadIdx.x];
    __syncthreads();
    if (wave < P)
        for (int b = lane; b < pl[wave].nq; b += 64) qt[wave][b] = gload<double>(pl[wave].qv, b);
    __syncthreads();
    const int pl_l = lane >> 3, g_l = lane & 7;
    const bool lane_on = pl_l < P && g_l < pl[pl_l].G;
    const int32_t* bd = lane_on ? pl[pl_l].bounds + (int64_t)g_l * (ntiles + 1) : nullptr;
    const int32_t gk_off = lane_on ? pl[pl_l].gk_off : 0, gb_off = lane_on ? pl[pl_l].gb_off : 0;
    uint8_t(*B)[kAggVTile] = bins[wave];
    uint32_t(*H)[kAggVTile / 32] = here[wave];
    unsigned bad = 0;
    int32_t nb0 = 0, nb1 = 0;
    auto fetch = [&](int64_t tt) {
        if (lane_on && tt < ntiles) {
            nb0 = gload<int32_t>(bd, tt);
            nb1 = gload<int32_t>(bd, tt + 1);
        }
    };
    // a tile's piece tables into buffer `buf`; returns its element count
    auto plan = [&](int buf, int32_t b0, int32_t b1, int ln) -> int {
        const int32_t len = lane_on && b1 > b0 ? b1 - b0 : 0;
        const int32_t x = (int32_t)wave_incl_scan_u32((uint32_t)len);
        pre[buf][wave][ln + 1] = x;
        if (ln == 0) pre[buf][wave][0] = 0;
        pk0[buf][wave][ln] = gk_off + b0;
        pn0[buf][wave][ln] = gb_off + b0;
        __builtin_amdgcn_wave_barrier();
        return __builtin_amdgcn_readlane(x, 63);
    };
    auto piece_of = [&](int buf, int j) -> int {  // largest s < 64 with pre[s] <= j
        int s_ = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
            if (pre[buf][wave][s_ + step] <= j) s_ += step;
        return s_;
    };
    auto load = [&](int buf, int total, int ln, int32_t (&kk)[kAggWPer], uint32_t (&bb)[kAggWPer]) {
        int spc[kAggWPer];
#pragma unroll
        for (int u = 0; u < kAggWPer; u++) {
            const int j = ln + 64 * u;
            spc[u] = piece_of(buf, j < total ? j : 0);
        }
#pragma unroll
        for (int u = 0; u < kAggWPer; u++) {
            const int j = ln + 64 * u;
            kk[u] = INT32_MIN;
            bb[u] = 0;
            if (j < total) {
                const int sp = spc[u], d = j - pre[buf][wave][sp];
                kk[u] = gload<int32_t>(kbase, (uint32_t)(pk0[buf][wave][sp] + d));
                bb[u] = gload<uint8_t>(bbase, (uint32_t)(pn0[buf][wave][sp] + d)) | ((uint32_t)(sp >> 3) << 8);
            }
        }
    };
    int64_t prev_k0 = -1, prev_nk = 0;
    double* T = reinterpret_cast<double*>(&B[0][0]);
    auto store_prev = [&](int l) {
        if (prev_k0 < 0) return;
        double* o = out + prev_k0;
        const bool whole = prev_nk == kAggVTile && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int x = 128 * q + 2 * l;
            const double2 v = *reinterpret_cast<const double2*>(T + x);
            if (whole) {
                *reinterpret_cast<double2*>(o + x) = v;
            } else {
                if (x < prev_nk) o[x] = v.x;
                if (x + 1 < prev_nk) o[x + 1] = v.y;
            }
        }
        __builtin_amdgcn_wave_barrier();
        prev_k0 = -1;
    };
    const TileWalk tw = tile_walk(blockIdx.x, gridDim.x, wave, kWaves, ntiles);
    int buf = 0, total = 0;
    int32_t kk[kAggWPer], kn[kAggWPer];
    uint32_t bb[kAggWPer], bn[kAggWPer];
    if (tw.t0 < tw.t1) {
        fetch(tw.t0);
        total = plan(0, nb0, nb1, lane);
        load(0, total, lane, kk, bb);
        fetch(tw.t0 + tw.step);
    }
    for (int64_t t = tw.t0; t < tw.t1; t += tw.step) {
        int ln = lane;  // lane-derived values rematerialised per tile (hoisted, they spill)
        asm volatile("" : "+v"(ln));
        const int64_t k0 = t << kAggVBits, nk = std::min<int64_t>(kAggVTile, dim - k0);
        // the next tile: its piece tables and its element loads, in flight while this one is summed
        int total_n = 0;
        const bool more = t + tw.step < tw.t1;
        if (more) {
            total_n = plan(buf ^ 1, nb0, nb1, ln);
            load(buf ^ 1, total_n, ln, kn, bn);
            fetch(t + 2 * tw.step);
        }
        store_prev(ln);
        reinterpret_cast<uint64_t*>(H)[ln] = 0;
        __builtin_amdgcn_wave_barrier();
        auto stage = [&](int p, int32_t k, uint32_t b) {
            if (k < k0 || (int64_t)k >= k0 + nk) {  // k_agg_bounds placed it here: an error
                bad |= 1u;
                return;
            }
            const int xk = (int)(k - k0);
            B[p][xk] = (uint8_t)b;
            const uint32_t bit = 1u << (xk & 31);
            if (atomicOr(&H[p][xk >> 5], bit) & bit) bad |= 2u;  // a key twice in one payload
        };
#pragma unroll
        for (int u = 0; u < kAggWPer; u++)
            if (ln + 64 * u < total) stage((int)(bb[u] >> 8), kk[u], bb[u] & 0xFFu);
        for (int j = 64 * kAggWPer + ln; j < total; j += 64) {  // elements past the registers
            const int sp = piece_of(buf, j), d = j - pre[buf][wave][sp];
            stage(sp >> 3, gload<int32_t>(kbase, (uint32_t)(pk0[buf][wave][sp] + d)),
                  gload<uint8_t>(bbase, (uint32_t)(pn0[buf][wave][sp] + d)));
        }
        __builtin_amdgcn_wave_barrier();
        double acc[8];
#pragma unroll
        for (int i = 0; i < 8; i++) acc[i] = from_out && 8 * ln + i < nk ? out[k0 + 8 * ln + i] : 0.0;
        for (int p = 0; p < P; p++) {
            const uint32_t m = reinterpret_cast<const uint8_t*>(H[p])[ln];
            const uint2 bw8 = *reinterpret_cast<const uint2*>(&B[p][8 * ln]);
            const bool dform = pl[p].dense_form != 0;
            double v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t b = ((i < 4 ? bw8.x : bw8.y) >> (8 * (i & 3))) & 0xFFu;
                v[i] = 0.0;
                if (m & (1u << i)) v[i] = qt[p][b];
            }
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if ((m & (1u << i)) && (!dform || fabs(v[i]) > 1e-8)) acc[i] += v[i];
                if (dform && __double_as_longlong(acc[i]) == (long long)0x8000000000000000ull) acc[i] = 0.0;
            }
        }
        if (scale != 1.0)
#pragma unroll
            for (int i = 0; i < 8; i++) acc[i] = __dmul_rn(acc[i], scale);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; q++)
            *reinterpret_cast<double2*>(T + 8 * ln + 2 * q) = make_double2(acc[2 * q], acc[2 * q + 1]);
        __builtin_amdgcn_wave_barrier();
        prev_k0 = k0;
        prev_nk = nk;
        buf ^= 1;
        total = total_n;
#pragma unroll
        for (int u = 0; u < kAggWPer; u++) {
            kk[u] = kn[u];
            bb[u] = bn[u];
        }
    }
    store_prev(lane);
    if (bad) atomicOr(err, bad);
}

#endif  // SKML_AB

// The sum tile itself in LDS: the waves, run pieces and prefetch of k_agg_vtiles_pf, but each
// element is added straight into the wave's tile of doubles (read, add, write back) instead of
// being staged as a bin and summed by a sweep over every (payload, key) slot, which looked up
// quantValues once per (payload, key) for ~10 % present.  The elements of a tile are concatenated
// payload by payload, so each element row (one load instruction) holds ascending payloads by lane
// and later rows never hold an earlier payload; a row is added payload by payload (one masked pass
// per payload present in it, usually one or two), and since a payload holds a key at most once, no
// two lanes of a pass touch the same slot and every key receives its payloads' values in payload
// order -- Gradient.sum's order, with the staged form's roundings.  A key repeated inside a
// payload (presence bit already set) is not added and sets err bit 2.  Dense-form payloads
// (DenseDoubleGradient.plusBy: only |v| > 1e-8 added, and every key's -0.0 sum turned into +0.0)
// sweep the tile once their payload is complete, before any later payload's add.
// BITS: 2^BITS keys per tile (512; 1,024-key tiles on four waves per workgroup, with run pieces
// twice as long, ran 5.7 against 5.0 ms for 8 C3 payloads: 247 VGPRs and half the waves per CU,
// profiles/ab/r05_agg_rmw1k.txt), PER: elements per lane held in registers (a longer tile takes
// the rest row by row).  DENSE: some payload of the launch takes the dense form.
// O / src: agg_tiles_w_body's.
template <int BITS, int WAVES, int PER, bool DENSE, typename O>
__device__ __forceinline__ void agg_rmw_body(
    const AggPayload* __restrict__ pays, int P, int64_t ntiles, int64_t dim, O* out, const double* src, int from_out,
    double scale, unsigned* __restrict__ err, const int32_t* __restrict__ kbase, const uint8_t* __restrict__ bbase) {
    constexpr int kTile = 1 << BITS, kKeys = kTile / 64;  // keys per lane in the stores
    static_assert(PER == 8 || PER == 16, "piece bytes written as 8 or 16");
    static_assert(kTile / 64 <= 16, "presence bits: 64 words of 16 bits at most");
    __shared__ __attribute__((aligned(16))) double tsum[WAVES][kTile];
    // presence bits of the payload being added: key x at word x % 64, bit x / 64, cleared at each
    // payload (a pass's random keys spread over 64 words: few lanes share a word's atomic)
    __shared__ uint32_t here[WAVES][64];
    __shared__ double qt[kAggPB][kAggLdsValues];
    __shared__ int32_t pre[2][WAVES][65];
    __shared__ int2 pkn[2][WAVES][64];  // piece s's key / bin element bases minus its first index pre[s]
    __shared__ __attribute__((aligned(16))) uint8_t pcs[WAVES][64 * PER];  // piece of element j
    __shared__ AggPayload pl[kAggPB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < P * (int)(sizeof(AggPayload) / 8))
        reinterpret_cast<uint64_t*>(pl)[threadIdx.x] = reinterpret_cast<const uint64_t*>(pays)[threadIdx.x];
    __syncthreads();
    for (int q = wave; q < P; q += WAVES)
        for (int b = lane; b < pl[q].nq; b += 64) qt[q][b] = gload<double>(pl[q].qv, b);
    __syncthreads();
    uint32_t dmask = 0;  // dense-form payloads
    if constexpr (DENSE) {
        for (int q = 0; q < P; q++) dmask |= pl[q].dense_form ? 1u << q : 0u;
        dmask = __builtin_amdgcn_readfirstlane(dmask);
    }
    const int pl_l = lane >> 3, g_l = lane & 7;
    const bool lane_on = pl_l < P && g_l < pl[pl_l].G;
    const int32_t* bd = lane_on ? pl[pl_l].bounds + (int64_t)g_l * (ntiles + 1) : nullptr;
    const int32_t gk_off = lane_on ? pl[pl_l].gk_off : 0, gb_off = lane_on ? pl[pl_l].gb_off : 0;
    double* T = tsum[wave];
    uint32_t* H = here[wave];
    unsigned bad = 0;
    int32_t nb0 = 0, nb1 = 0;
    auto fetch = [&](int64_t tt) {
        if (lane_on && tt < ntiles) {
            nb0 = gload<int32_t>(bd, tt);
            nb1 = gload<int32_t>(bd, tt + 1);
        }
    };
    auto plan = [&](int buf, int32_t b0, int32_t b1, int ln) -> int {
        const int32_t len = lane_on && b1 > b0 ? b1 - b0 : 0;
        const int32_t x = (int32_t)wave_incl_scan_u32((uint32_t)len);
        pre[buf][wave][ln + 1] = x;
        if (ln == 0) pre[buf][wave][0] = 0;
        pkn[buf][wave][ln] = make_int2(gk_off + b0 - (x - len), gb_off + b0 - (x - len));
        __builtin_amdgcn_wave_barrier();
        return __builtin_amdgcn_readlane(x, 63);
    };
    auto piece_of = [&](int buf, int j) -> int {  // largest s < 64 with pre[s] <= j
        int s_ = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
            if (pre[buf][wave][s_ + step] <= j) s_ += step;
        return s_;
    };
    // the pieces of the elements held in registers: lane l writes its own piece's number over the
    // piece's elements in pcs (a piece holds ~6-13 elements of a C3 tile: stores, no dependent
    // LDS reads); the loads then read the piece of j = l + 64 u back
    auto load = [&](int buf, int total, int ln, int32_t (&kk)[PER], uint32_t (&bb)[PER]) {
        {
            const int e0 = pre[buf][wave][ln], e1 = min(pre[buf][wave][ln + 1], 64 * PER);
            for (int e = e0; e < e1; e++) pcs[wave][e] = (uint8_t)ln;
            __builtin_amdgcn_wave_barrier();
        }
        int spc[PER];
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int j = ln + 64 * u;
            spc[u] = j < total ? (int)pcs[wave][j] : 0;
        }
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int j = ln + 64 * u;
            kk[u] = INT32_MIN;
            bb[u] = 0;
            if (j < total) {
                const int sp = spc[u];
                const int2 kb = pkn[buf][wave][sp];
                kk[u] = gload<int32_t>(kbase, (uint32_t)(kb.x + j));
                bb[u] = gload<uint8_t>(bbase, (uint32_t)(kb.y + j)) | ((uint32_t)(sp >> 3) << 8);
            }
        }
    };
    int64_t prev_k0 = -1, prev_nk = 0;
    auto store_prev = [&](int l) {  // the previous tile's sums, x scale, 1 KB per store instruction
        if (prev_k0 < 0) return;
        O* o = out + prev_k0;
        const bool whole = prev_nk == kTile && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
        if constexpr (!std::is_same<O, double>::value) {  // kV values per lane and store instruction
            constexpr int kV = agg_out_vec<O>();
            static_assert(kTile % (64 * kV) == 0, "whole rows of 16-byte stores: a smaller tile would store nothing");
#pragma unroll
            for (int q = 0; q < kTile / (64 * kV); q++) {
                const int x = 64 * kV * q + kV * l;
                double v[kV];
#pragma unroll
                for (int i = 0; i < kV; i += 2) {
                    const double2 d = *reinterpret_cast<const double2*>(T + x + i);
                    v[i] = scale != 1.0 ? __dmul_rn(d.x, scale) : d.x;
                    v[i + 1] = scale != 1.0 ? __dmul_rn(d.y, scale) : d.y;
                }
                if (whole) {
                    agg_store_vec<O>(o, x, v);
                } else {
#pragma unroll
                    for (int i = 0; i < kV; i++)
                        if (x + i < prev_nk) store_narrow<O>(o, x + i, (float)v[i]);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < kTile / 128; q++) {
                const int x = 128 * q + 2 * l;
                double2 v = *reinterpret_cast<const double2*>(T + x);
                if (scale != 1.0) {
                    v.x = __dmul_rn(v.x, scale);
                    v.y = __dmul_rn(v.y, scale);
                }
#ifdef SKML_ABLATE_AGG_STORE  // timing ablation only (no sums written): the sum's stores priced
                if (v.x == 12345.678) o[x] = v.y;
                continue;
#endif
                if (whole) {
                    *reinterpret_cast<double2*>(o + x) = v;
                } else {
                    if (x < prev_nk) o[x] = v.x;
                    if (x + 1 < prev_nk) o[x + 1] = v.y;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        prev_k0 = -1;
    };
    // payloads [a, b) complete: a dense-form one among them turns every -0.0 sum of the tile into +0.0
    auto finish = [&](int a, int b, int ln) {
        if constexpr (!DENSE) return;
        if (b <= a || !((dmask >> a) & ((1u << (b - a)) - 1u))) return;  // wave-uniform
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < kKeys; i++) {
            double& t = T[kKeys * ln + i];
            if (__double_as_longlong(t) == (long long)0x8000000000000000ull) t = 0.0;
        }
        __builtin_amdgcn_wave_barrier();
    };
    const TileWalk tw = tile_walk_xcd(blockIdx.x, gridDim.x, wave, WAVES, ntiles);
    int buf = 0, total = 0;
    int32_t kk[PER], kn[PER];
    uint32_t bb[PER], bn[PER];
    if (tw.t0 < tw.t1) {
        fetch(tw.t0);
        total = plan(0, nb0, nb1, lane);
        load(0, total, lane, kk, bb);
        fetch(tw.t0 + tw.step);
    }
    for (int64_t t = tw.t0; t < tw.t1; t += tw.step) {
        int ln = lane;  // lane-derived values rematerialised per tile (hoisted, they spill)
        asm volatile("" : "+v"(ln));
        const int64_t k0 = t << BITS, nk = std::min<int64_t>(kTile, dim - k0);
        int total_n = 0;
        const bool more = t + tw.step < tw.t1;
        if (more) {
            total_n = plan(buf ^ 1, nb0, nb1, ln);
            load(buf ^ 1, total_n, ln, kn, bn);
            fetch(t + 2 * tw.step);
        }
        store_prev(ln);
        // the tile's starting sums (a later batch of payloads continues them)
#pragma unroll
        for (int q = 0; q < kKeys / 2; q++) {
            double2 v = make_double2(0.0, 0.0);
            if (from_out) {
                const int x = kKeys * ln + 2 * q;
                if (x < nk) v.x = src[k0 + x];
                if (x + 1 < nk) v.y = src[k0 + x + 1];
            }
            *reinterpret_cast<double2*>(T + kKeys * ln + 2 * q) = v;
        }
        __builtin_amdgcn_wave_barrier();
        int h_for = -1, p_act = 0;  // H's payload; payloads below p_act are complete (wave-uniform)
        const int32_t k0i = (int32_t)k0;  // dim <= 2^31: tile starts fit int32
        // one row of elements (lane l: element j = l + 64 u), payload by payload
        auto add_row = [&](bool act, int p_el, int32_t k, uint32_t b) {
            uint64_t rem = __ballot(act);
            while (rem) {
                const int first = __ffsll((unsigned long long)rem) - 1;
                const int pcur = __builtin_amdgcn_readlane(p_el, first);
                if (pcur != h_for) {  // a new payload: the ones before it are complete
                    finish(p_act, pcur, ln);
                    p_act = pcur;
                    H[ln] = 0u;
                    __builtin_amdgcn_wave_barrier();
                    h_for = pcur;
                }
                const bool mine = act && p_el == pcur;
#ifdef SKML_ABLATE_AGG_RMW  // timing ablation only (wrong sums): the adds into the tile priced
                if (mine && k == INT32_MIN) bad |= 4u;
                rem &= ~__ballot(mine);
                continue;
#endif
                if (mine) {
                    const int32_t xk = k - k0i;
                    if ((uint32_t)xk >= (uint32_t)nk) {  // outside the tile its bounds placed it in: an error
                        bad |= 1u;
                    } else {
                        const uint32_t bit = 1u << (xk >> 6);
                        if (atomicOr(&H[xk & 63], bit) & bit) {
                            bad |= 2u;  // a key twice in one payload
                        } else {
                            const double v = qt[pcur][b];
                            if (!DENSE || !((dmask >> pcur) & 1u) || fabs(v) > 1e-8) T[xk] = T[xk] + v;
                        }
                    }
                }
                rem &= ~__ballot(mine);
            }
        };
#pragma unroll
        for (int u = 0; u < PER; u++)
            add_row(ln + 64 * u < total, (int)(bb[u] >> 8), kk[u], bb[u] & 0xFFu);
        for (int j0 = 64 * PER; j0 < total; j0 += 64) {  // rows past the registers
            const int j = j0 + ln;
            const bool act = j < total;
            int sp = 0;
            int2 kb = make_int2(0, 0);
            if (act) {
                sp = piece_of(buf, j);
                kb = pkn[buf][wave][sp];
            }
            const int32_t k = act ? gload<int32_t>(kbase, (uint32_t)(kb.x + j)) : 0;
            const uint32_t b = act ? gload<uint8_t>(bbase, (uint32_t)(kb.y + j)) : 0u;
            add_row(act, sp >> 3, k, b);
        }
        finish(p_act, P, ln);  // the payloads from the last one seen on
        __builtin_amdgcn_wave_barrier();
        prev_k0 = k0;
        prev_nk = nk;
        buf ^= 1;
        total = total_n;
#pragma unroll
        for (int u = 0; u < PER; u++) {
            kk[u] = kn[u];
            bb[u] = bn[u];
        }
    }
    store_prev(lane);
    if (bad) atomicOr(err, bad);
}
template <int BITS, int WAVES, int PER, bool DENSE>
__global__ __launch_bounds__(64 * WAVES) void k_agg_rmw(
    const AggPayload* __restrict__ pays, int P, int64_t ntiles, int64_t dim, double* __restrict__ out, int from_out,
    double scale, unsigned* __restrict__ err, const int32_t* __restrict__ kbase, const uint8_t* __restrict__ bbase) {
    agg_rmw_body<BITS, WAVES, PER, DENSE, double>(pays, P, ntiles, dim, out, out, from_out, scale, err, kbase, bbase);
}
template <int BITS, int WAVES, int PER, bool DENSE, typename O>
__global__ __launch_bounds__(64 * WAVES) void k_agg_rmw_o(
    const AggPayload* __restrict__ pays, int P, int64_t ntiles, int64_t dim, O* __restrict__ out,
    const double* __restrict__ src, int from_out, double scale, unsigned* __restrict__ err,
    const int32_t* __restrict__ kbase, const uint8_t* __restrict__ bbase) {
    agg_rmw_body<BITS, WAVES, PER, DENSE, O>(pays, P, ntiles, dim, out, src, from_out, scale, err, kbase, bbase);
}

// The staged wave-tile form is the default for payloads of at most 8 groups and 256 quantValues
// (the caller launches it 8 payloads at a time); the wave-per-payload tiles take every other shape
// (SKML_FORM_AGG_TILES forces them for tests).
bool agg_vtiles_ok(int max_groups, int max_nq) {
    return max_groups <= 8 && max_nq <= kAggLdsValues && form(SKML_FORM_AGG_TILES) != 1;
}
int agg_tile_bits(bool vtiles) { return vtiles ? kAggVBits : 12; }

hipError_t launch_agg_tiles(hipStream_t st, const AggPayload* pays, int P, int64_t ntiles, int64_t dim, double* out,
                            int from_out, double scale, unsigned* err, bool vtiles, const int32_t* kbase,
                            const uint8_t* bbase, bool any_dense) {
    if (ntiles <= 0) return hipSuccess;
    if (vtiles) {
        if (P < 1 || P > kAggVPayloads) return hipErrorInvalidValue;  // one lane per (payload, group)
        // the default: the sum tile in LDS (k_agg_rmw); the A/B build adds SKML_FORM_AGG_TILES 4 / 5
        // (the staged tiles with and without the next tile's prefetch; 5.57-5.64 against 5.63-5.66
        // ms for 8 C3 payloads, profiles/ab/r05_pf.txt, both slower than k_agg_rmw) and 2 / 3 (four /
        // two staged tiles per wave round)
#ifdef SKML_AB
        const int f = form(SKML_FORM_AGG_TILES);
        if (f >= 2 && f <= 5) {
            if (f == 4) {
                static const int resident_pf = resident_blocks(k_agg_vtiles_pf, kAggThreads);
                const int64_t all = sp_tiles(ntiles, kAggThreads / 64);
                const unsigned grid = (unsigned)(resident_pf <= 0 ? all : std::min<int64_t>(all, resident_pf));
                hipLaunchKernelGGL(k_agg_vtiles_pf, dim3(grid), dim3(kAggThreads), 0, st, pays, P, ntiles, dim, out,
                                   from_out, scale, err, kbase, bbase);
                return hipGetLastError();
            }
#define SKML_VT_LAUNCH(SUB)                                                                                  \
    do {                                                                                                     \
        static const int res = resident_blocks(k_agg_vtiles<SUB>, kAggThreads);                               \
        const int64_t all = sp_tiles(sp_tiles(ntiles, SUB), kAggThreads / 64);                               \
        const unsigned grid = (unsigned)(res <= 0 ? all : std::min<int64_t>(all, res));                      \
        hipLaunchKernelGGL(k_agg_vtiles<SUB>, dim3(grid), dim3(kAggThreads), 0, st, pays, P, ntiles, dim, out, \
                           from_out, scale, err, kbase, bbase);                                              \
    } while (0)
            if (f == 2) SKML_VT_LAUNCH(4);
            else if (f == 3) SKML_VT_LAUNCH(2);
            else SKML_VT_LAUNCH(1);
#undef SKML_VT_LAUNCH
            return hipGetLastError();
        }
#endif
#define SKML_RMW_LAUNCH(DENSE)                                                                                   \
    do {                                                                                                         \
        static const int res = resident_blocks(k_agg_rmw<kAggVBits, 8, 8, DENSE>, kAggThreads);                   \
        const int64_t all = sp_tiles(ntiles, 8);                                                                 \
        const unsigned grid = (unsigned)(res <= 0 ? all : std::min<int64_t>(all, res));                          \
        hipLaunchKernelGGL((k_agg_rmw<kAggVBits, 8, 8, DENSE>), dim3(grid), dim3(kAggThreads), 0, st, pays, P,   \
                           ntiles, dim, out, from_out, scale, err, kbase, bbase);                                \
    } while (0)
        if (any_dense) SKML_RMW_LAUNCH(true);
        else SKML_RMW_LAUNCH(false);
#undef SKML_RMW_LAUNCH
        return hipGetLastError();
    }
    // persistent: as many workgroups as are resident at once
    static const int resident = resident_blocks(k_agg_tiles_w, kAggThreads);
    const unsigned grid = (unsigned)(resident <= 0 ? ntiles : std::min<int64_t>(ntiles, resident));
    hipLaunchKernelGGL(k_agg_tiles_w, dim3(grid), dim3(kAggThreads), 0, st, pays, P, ntiles, dim, out, from_out, scale,
                       err);
    return hipGetLastError();
}

// The last launch of a sum returned as float / bf16 / fp16: the default forms of launch_agg_tiles
// (no A/B forms), continued from the doubles of `src` when from_out.
template <typename O>
hipError_t launch_agg_tiles_o(hipStream_t st, const AggPayload* pays, int P, int64_t ntiles, int64_t dim, O* out,
                              const double* src, int from_out, double scale, unsigned* err, bool vtiles,
                              const int32_t* kbase, const uint8_t* bbase, bool any_dense) {
    if (ntiles <= 0) return hipSuccess;
    if (from_out && !src) return hipErrorInvalidValue;
    if (vtiles) {
        if (P < 1 || P > kAggVPayloads) return hipErrorInvalidValue;
#define SKML_RMW_LAUNCH(DENSE)                                                                                   \
    do {                                                                                                         \
        static const int res = resident_blocks(k_agg_rmw_o<kAggVBits, 8, 8, DENSE, O>, kAggThreads);              \
        const int64_t all = sp_tiles(ntiles, 8);                                                                 \
        const unsigned grid = (unsigned)(res <= 0 ? all : std::min<int64_t>(all, res));                          \
        hipLaunchKernelGGL((k_agg_rmw_o<kAggVBits, 8, 8, DENSE, O>), dim3(grid), dim3(kAggThreads), 0, st, pays, \
                           P, ntiles, dim, out, src, from_out, scale, err, kbase, bbase);                        \
    } while (0)
        if (any_dense) SKML_RMW_LAUNCH(true);
        else SKML_RMW_LAUNCH(false);
#undef SKML_RMW_LAUNCH
        return hipGetLastError();
    }
    static const int resident = resident_blocks(k_agg_tiles_w_o<O>, kAggThreads);
    const unsigned grid = (unsigned)(resident <= 0 ? ntiles : std::min<int64_t>(ntiles, resident));
    hipLaunchKernelGGL(k_agg_tiles_w_o<O>, dim3(grid), dim3(kAggThreads), 0, st, pays, P, ntiles, dim, out, src,
                       from_out, scale, err);
    return hipGetLastError();
}
hipError_t launch_agg_tiles_f32(hipStream_t st, const AggPayload* pays, int P, int64_t ntiles, int64_t dim, float* out,
                                const double* src, int from_out, double scale, unsigned* err, bool vtiles,
                                const int32_t* kbase, const uint8_t* bbase, bool any_dense) {
    return launch_agg_tiles_o<float>(st, pays, P, ntiles, dim, out, src, from_out, scale, err, vtiles, kbase, bbase,
                                     any_dense);
}
hipError_t launch_agg_tiles_bf16(hipStream_t st, const AggPayload* pays, int P, int64_t ntiles, int64_t dim,
                                 bf16_t* out, const double* src, int from_out, double scale, unsigned* err, bool vtiles,
                                 const int32_t* kbase, const uint8_t* bbase, bool any_dense) {
    return launch_agg_tiles_o<bf16_t>(st, pays, P, ntiles, dim, out, src, from_out, scale, err, vtiles, kbase, bbase,
                                      any_dense);
}
hipError_t launch_agg_tiles_f16(hipStream_t st, const AggPayload* pays, int P, int64_t ntiles, int64_t dim, f16_t* out,
                                const double* src, int from_out, double scale, unsigned* err, bool vtiles,
                                const int32_t* kbase, const uint8_t* bbase, bool any_dense) {
    return launch_agg_tiles_o<f16_t>(st, pays, P, ntiles, dim, out, src, from_out, scale, err, vtiles, kbase, bbase,
                                     any_dense);
}

// live entries (|quantValues[bin]| > 1e-8) of a restored payload, for toAuto's dense / sparse choice
template <typename B>
__global__ __launch_bounds__(kSpThreads) void k_count_live(const B* __restrict__ bins, int64_t n,
                                                           const double* __restrict__ qv,
                                                           unsigned long long* __restrict__ count) {
    uint64_t c = 0;
    for (int64_t i = (int64_t)blockIdx.x * kSpThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSpThreads)
        c += fabs(qv[bins[i]]) > 1e-8 ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}
hipError_t launch_count_live(hipStream_t st, const void* bins, int bw, int64_t n, const double* qv, uint64_t* count) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(uint64_t), st);
    if (e != hipSuccess || n <= 0) return e;
    const int64_t grid = std::min<int64_t>(sp_tiles(n, kSpThreads * 8), 4096);
    if (bw == 1)
        hipLaunchKernelGGL(k_count_live<uint8_t>, dim3((unsigned)grid), dim3(kSpThreads), 0, st,
                           static_cast<const uint8_t*>(bins), n, qv, reinterpret_cast<unsigned long long*>(count));
    else
        hipLaunchKernelGGL(k_count_live<uint16_t>, dim3((unsigned)grid), dim3(kSpThreads), 0, st,
                           static_cast<const uint16_t*>(bins), n, qv, reinterpret_cast<unsigned long long*>(count));
    return hipGetLastError();
}

// =============================================================================================
// Merge rounds: runs r = [rs[r], rs[r+1]); pairs (2q, 2q+1) merge into the same range, ties
// take the lower run first (Sort.merge scans heads in list order with a strict `<`).
// Each thread produces kMergePer outputs found by a merge-path search.
// =============================================================================================
constexpr int kMergePer = 8;

__device__ __forceinline__ int64_t merge_path(const int32_t* A, int64_t na, const int32_t* B, int64_t nb, int64_t d) {
    int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A[mid] <= B[d - mid - 1]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// merge_path by one wave: each step probes 64 evenly spaced points of the remaining range (the
// predicate A[i] <= B[d-i-1] is true then false along i), so a run of 13 M keys takes 4 dependent
// global reads instead of 24.
__device__ __forceinline__ int64_t merge_path_wave(const int32_t* A, int64_t na, const int32_t* B, int64_t nb,
                                                   int64_t d, int lane) {
    int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (hi - lo > 64) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t i = lo + (int64_t)lane * step;
        const bool p = i < hi && A[i] <= B[d - i - 1];
        const int c = __popcll(__ballot(p));
        if (c == 0) return lo;
        const int64_t nlo = lo + (int64_t)(c - 1) * step + 1, nhi = lo + (int64_t)c * step;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    const int64_t i = lo + lane;
    const bool p = i < hi && A[i] <= B[d - i - 1];
    return lo + __popcll(__ballot(p));
}

// The round's run offsets by value (kernel arguments: no dependent loads before the searches).
struct MergeRuns {
    int64_t r[kMaxGroups + 1];
};
constexpr int kMergeTile = 4096, kMergeThreads = 512;  // outputs and threads per merge workgroup
static_assert(kMergeTile == kMergePer * kMergeThreads, "8 outputs per thread");

// Split points of the merge paths at every tile boundary (outputs b * kMergeTile, b in [0, tiles]),
// one wave per boundary: split[b] = how many of the boundary's pair's lower run precede it.
__global__ __launch_bounds__(256) void k_merge_splits(const int32_t* __restrict__ kin, MergeRuns rs, int nruns,
                                                      int64_t total, int64_t nb_bounds, int64_t* __restrict__ split) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nb_bounds) return;
    const int64_t pos = std::min<int64_t>(b * kMergeTile, total);
    int q = 0;  // the pair holding pos: the last even run start <= pos (runs [rs[2q], rs[2q+2]))
    while (2 * q + 2 < nruns && rs.r[2 * q + 2] <= pos) q++;
    const int64_t a0 = rs.r[2 * q], a1 = rs.r[std::min(2 * q + 1, nruns)], b1 = rs.r[std::min(2 * q + 2, nruns)];
    int64_t ia = 0;
    if (pos > a0) ia = pos >= b1 ? a1 - a0 : merge_path_wave(kin + a0, a1 - a0, kin + a1, b1 - a1, pos - a0, lane);
    if (lane == 0) split[b] = ia;
}

// One workgroup per kMergeTile outputs: the tile's end points on its pairs' merge paths come from
// k_merge_splits (or are a pair's ends), the tile's A and B pieces are staged in LDS (coalesced),
// every thread merges 8 outputs from its LDS merge-path split into an LDS output tile, and the tile
// is stored coalesced.
__global__ __launch_bounds__(kMergeThreads) void k_merge_round(const int32_t* __restrict__ kin,
                                                               const int32_t* __restrict__ bin_in,
                                                               int32_t* __restrict__ kout, int32_t* __restrict__ bout,
                                                               MergeRuns rs, int nruns, int64_t total,
                                                               const int64_t* __restrict__ split) {
    __shared__ int32_t sk[kMergeTile], sb[kMergeTile], ok[kMergeTile], ob[kMergeTile];
    const int t = threadIdx.x;
    const int64_t o0 = (int64_t)blockIdx.x * kMergeTile;
    const int64_t o1 = std::min<int64_t>(o0 + kMergeTile, total);
    const int64_t sp0 = split[blockIdx.x], sp1 = split[blockIdx.x + 1];
    int q = 0;
    for (int64_t out = o0; out < o1;) {
        while (2 * q + 2 <= nruns && rs.r[2 * q + 2] <= out) q++;
        const int64_t a0 = rs.r[2 * q];
        const int64_t a1 = rs.r[std::min(2 * q + 1, nruns)];
        const int64_t b1 = rs.r[std::min(2 * q + 2, nruns)];
        const int64_t na = a1 - a0;
        const int64_t end = std::min(o1, b1);
        // a segment starts at the tile start or at a pair start, and ends at the tile end or a pair end
        const int64_t ia0 = out == a0 ? 0 : sp0;
        const int64_t ia1 = end == b1 ? na : sp1;
        const int64_t ib0 = (out - a0) - ia0, ib1 = (end - a0) - ia1;
        const int la = (int)(ia1 - ia0), lb = (int)(ib1 - ib0);
        for (int k = t; k < la + lb; k += kMergeThreads) {
            const int64_t src = k < la ? a0 + ia0 + k : a1 + ib0 + (k - la);
            sk[k] = kin[src];
            sb[k] = bin_in[src];
        }
        __syncthreads();
        const int d = t * kMergePer;
        if (d < la + lb) {
            int ia = (int)merge_path(sk, la, sk + la, lb, d), ib = d - ia;
            const int cnt = std::min(kMergePer, la + lb - d);
            for (int j = 0; j < cnt; j++) {
                const bool takeA = ib >= lb || (ia < la && sk[ia] <= sk[la + ib]);
                const int k = takeA ? ia++ : la + ib++;
                ok[d + j] = sk[k];
                ob[d + j] = sb[k];
            }
        }
        __syncthreads();
        // the merged segment leaves with consecutive lanes on consecutive addresses (a thread's
        // own 8 outputs would be 32-byte strided stores)
        for (int k = t; k < la + lb; k += kMergeThreads) {
            kout[out + k] = ok[k];
            bout[out + k] = ob[k];
        }
        __syncthreads();
        out = end;
    }
}

hipError_t launch_merge_round(hipStream_t st, const int32_t* kin, const int32_t* bin_in, int32_t* kout,
                              int32_t* bout, const int64_t* run_start, int nruns, int64_t total, int64_t* split) {
    if (total <= 0) return hipSuccess;
    if (nruns > kMaxGroups) return hipErrorInvalidValue;
    MergeRuns rs{};
    for (int i = 0; i <= nruns; i++) rs.r[i] = run_start[i];
    const int64_t tiles = sp_tiles(total, kMergeTile), nb = tiles + 1;
    hipLaunchKernelGGL(k_merge_splits, dim3((unsigned)sp_tiles(nb, 4)), dim3(256), 0, st, kin, rs, nruns, total, nb,
                       split);
    hipLaunchKernelGGL(k_merge_round, dim3((unsigned)tiles), dim3(kMergeThreads), 0, st, kin, bin_in, kout, bout, rs,
                       nruns, total, split);
    return hipGetLastError();
}

// ---- Sort.merge in one pass over key ranges (the regular case) ----
// Sort.merge (util/Sort.java:362-379) takes the smallest head of the G runs each step (ties to the
// lower run).  When every run ascends strictly, no key repeats across runs and every key lies in
// [0, INT32_MAX), that is the ascending order of all keys, so an element's output index is the
// number of keys smaller than its own.  k_rs_bounds records where each run enters every range of
// kRsRange keys (and flags a run that does not ascend or a key outside the range); k_rs_merge marks
// one range's keys in an LDS bitmap, scans the bitmap's popcounts, and sends each element to the
// range's base + its rank among the set bits, with its bin or quantValues[bin].  A repeated key
// (a bit already set) flags the input too, and the host then runs the pairwise merge rounds,
// which follow Sort.merge for any input.  Regular C3 payloads: one pass instead of three rounds.
#ifdef SKML_AB  // the ranges' bounds in a pass of their own (SKML_FORM_RUN_BOUNDS = 1); the key query writes them
__global__ __launch_bounds__(kSpThreads) void k_rs_bounds(const int32_t* __restrict__ gk, int64_t n,
                                                          const SpGroups* __restrict__ gp, int32_t* __restrict__ bounds,
                                                          RsInfo* __restrict__ info) {
    __shared__ int64_t S[kMaxGroups + 1];
    load_starts(gp, S);
    __syncthreads();
    unsigned bad = 0;
    run_bounds16<false>(gk, n, S, bounds, kRsRanges + 1, 0, 0, info, bad);
    if (bad) atomicOr(&info->irregular, 1u);
}

#endif  // SKML_AB

template <typename V>
__device__ __forceinline__ V rs_value(int32_t b, const V* lut, const double* qv, int nq, bool lds, unsigned& bad) {
    if constexpr (std::is_same<V, int32_t>::value) {
        return b;
    } else {
        if (b < 0 || b >= nq) {
            bad = 1;
            return (V)0;
        }
        return lds ? lut[b] : (V)qv[b];
    }
}

constexpr int kRsThreads = 256, kRsBatch = 4, kRsLut = 1024;
static_assert(kRsWords == kRsThreads, "one bitmap word per thread");
#ifdef SKML_AB  // the one-pass merge without the pipelining (SKML_FORM_RS_ROUNDS = 2), measured slower
template <typename V>
__global__ __launch_bounds__(kRsThreads) void k_rs_merge(const int32_t* __restrict__ gk, const int32_t* __restrict__ gb,
                                                         const SpGroups* __restrict__ gp,
                                                         const int32_t* __restrict__ bounds, RsInfo* __restrict__ info,
                                                         int32_t* __restrict__ keys_out, V* __restrict__ out,
                                                         const double* __restrict__ qv, int nq) {
    constexpr int kLut = std::is_same<V, int32_t>::value ? 1 : kRsLut;
    __shared__ uint32_t bm[kRsWords];
    __shared__ int32_t slot[kRsRange];  // the bin of the key at each offset of the range
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ int64_t lo_s[kMaxGroups];
    __shared__ int32_t pre[kMaxGroups + 1];
    __shared__ int64_t obase;
    __shared__ uint32_t wsum[kRsThreads / 64];
    __shared__ V lut[kLut];
    if (info->irregular) return;  // workgroup-uniform: the merge rounds run instead
    const int tmax = info->tmax1 - 1;
    const int G = gp->G, t_ = threadIdx.x, lane = t_ & 63, w = t_ >> 6;
    load_starts(gp, S);
    const bool lds = !std::is_same<V, int32_t>::value && nq <= kLut;
    if (lds)
        for (int b = t_; b < nq; b += kRsThreads) lut[b] = (V)qv[b];
    constexpr int64_t ld = kRsRanges + 1;
    unsigned bad = 0;
    // wave 0, lane g < G: run g's last range, and the bounds of this workgroup's next range,
    // loaded one range ahead so a range waits on one memory round trip (its elements), not two
    const int tl = (w == 0 && lane < G) ? info->tlast1[lane] - 1 : -1;  // -1: an empty run
    int32_t nlo = 0, nhi = 0;
    auto fetch = [&](int64_t tt) {
        if (tl >= 0 && tt <= tl) {
            nlo = bounds[(int64_t)lane * ld + tt];
            nhi = bounds[(int64_t)lane * ld + tt + 1];
        }
    };
    if (w == 0 && lane < G) fetch(blockIdx.x);
    for (int64_t t = blockIdx.x; t <= tmax; t += gridDim.x) {
        const int32_t clo = nlo, chi = nhi;
        if (w == 0 && lane < G) fetch(t + gridDim.x);
        __syncthreads();  // S / lut loaded; the previous range is done with bm / slot / pre
        if (w == 0) {  // lane g: run g's piece of this range
            int64_t lo = 0, len = 0, before = 0;
            if (lane < G) {
                const int64_t s0 = S[lane], s1 = S[lane + 1];
                lo = s1;
                int64_t hi = s1;
                if (tl >= 0 && t <= tl) {
                    lo = clo;
                    hi = chi;
                }
                before = lo - s0;
                len = hi - lo;
                lo_s[lane] = lo;
            }
            int64_t x = len;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int64_t y = __shfl_up(x, off, 64);
                if (lane >= off) x += y;
            }
            if (lane < kMaxGroups) pre[lane + 1] = (int32_t)x;
            if (lane == 0) pre[0] = 0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) before += __shfl_xor(before, off, 64);
            if (lane == 0) obase = before;
        }
        bm[t_] = 0;
        __syncthreads();
        const int cnt = pre[G];
        if (cnt == 0) continue;  // workgroup-uniform
        // the run holding j: with at most 8 runs a count of the run ends (in registers) at or below
        // j, else a binary search of the prefix
        int32_t re[8];
#pragma unroll
        for (int q = 0; q < 8; q++) re[q] = q + 1 <= G ? pre[q + 1] : INT32_MAX;
        auto run_of = [&](int j) -> int {
            if (G <= 8) {
                int g = 0;
#pragma unroll
                for (int q = 0; q < 8; q++) g += re[q] <= j ? 1 : 0;
                return g;
            }
            return agg_search32(pre, G, j);
        };
        // pass 1: the range's keys into the bitmap, their bins into the offset slots (4 loads of
        // each in flight per thread)
        for (int j0 = 0; j0 < cnt; j0 += kRsThreads * kRsBatch) {
            int32_t kk[kRsBatch], bb[kRsBatch];
#pragma unroll
            for (int u = 0; u < kRsBatch; u++) {
                const int j = j0 + u * kRsThreads + t_;
                kk[u] = -1;
                if (j < cnt) {
                    const int g = run_of(j);
                    const int64_t i = lo_s[g] + (j - pre[g]);
                    kk[u] = gk[i];
                    bb[u] = gb[i];
                }
            }
#pragma unroll
            for (int u = 0; u < kRsBatch; u++) {
                if (kk[u] < 0) continue;
                const uint32_t off = (uint32_t)kk[u] & (kRsRange - 1), bit = 1u << (off & 31);
                if (atomicOr(&bm[off >> 5], bit) & bit) bad = 1;  // a repeated key
                slot[off] = bb[u];
            }
        }
        __syncthreads();
        // pass 2: thread t_ owns bitmap word t_, i.e. the keys t * kRsRange + 32 t_ + [0, 32): its
        // set bits go out in key order from its exclusive popcount prefix
        const uint32_t word = bm[t_];
        const uint32_t own = __popc(word);
        uint32_t inc = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(inc, off, 64);
            if (lane >= off) inc += y;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        uint32_t run = inc - own;
        for (int q = 0; q < w; q++) run += wsum[q];
        int64_t o = obase + run;
        const int32_t kbase = (int32_t)(t * kRsRange) + 32 * t_;
        for (uint32_t m = word; m; m &= m - 1, o++) {
            const int b = __ffs(m) - 1;
            keys_out[o] = kbase + b;
            out[o] = rs_value<V>(slot[32 * t_ + b], lut, qv, nq, lds, bad);
        }
    }
    if (bad) atomicOr(&info->irregular, 2u);
}

#endif  // SKML_AB

// Sort.merge in one pass, software pipelined: while range t is marked, scanned and emitted, the
// element loads of the workgroup's next range are in flight (its piece table computed one range
// ahead into the other half of a double buffer, its run bounds fetched two ranges ahead).  The
// emission is coalesced: each thread lists its word's set offsets at their ranks in `ord`, and
// output j of the range is written by thread j % 256 (the per-bit stores of k_rs_merge write 64
// scattered words per instruction).  Values restores hold the bins as 16-bit slots (checked
// against nq on load: a bin outside quantValues flags the input, as rs_value does), so `ord` fits
// in the LDS the int32 slots took.  Same output and irregular-input flags as k_rs_merge.
// NARROW (values restores with at most 256 quantValues): byte slots and a 256-entry table, 26-27 KB
// of LDS instead of 37-41 KB, so 5-6 workgroups per CU hold ranges in flight instead of 3-4.
template <typename V, bool NARROW = false>
__global__ __launch_bounds__(kRsThreads) void k_rs_merge_pf(const int32_t* __restrict__ gk,
                                                            const int32_t* __restrict__ gb,
                                                            const SpGroups* __restrict__ gp,
                                                            const int32_t* __restrict__ bounds,
                                                            RsInfo* __restrict__ info, int32_t* __restrict__ keys_out,
                                                            V* __restrict__ out, const double* __restrict__ qv, int nq) {
    constexpr bool kBins = std::is_same<V, int32_t>::value;  // int32 bins out: any table value
    static_assert(!(kBins && NARROW), "narrow slots hold quantValues indices only");
    constexpr int kLut = kBins ? 1 : NARROW ? 256 : kRsLut;
    using ST = typename std::conditional<kBins, int32_t, typename std::conditional<NARROW, uint8_t, uint16_t>::type>::type;
    __shared__ uint32_t bm[kRsWords];
    __shared__ ST slot[kRsRange];
    __shared__ uint16_t ord[kRsRange];  // the range's set offsets in key order
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ int64_t lo_s[3][kMaxGroups];
    __shared__ int32_t pre[3][kMaxGroups + 1];
    __shared__ int64_t obase[3];
    __shared__ uint32_t wsum[kRsThreads / 64];
    __shared__ V lut[kLut];
    if (info->irregular) return;  // workgroup-uniform: the merge rounds run instead
    const int tmax = info->tmax1 - 1;
    const int G = gp->G, t_ = threadIdx.x, lane = t_ & 63, w = t_ >> 6;
    load_starts(gp, S);
    const bool lds = !std::is_same<V, int32_t>::value && nq <= kLut;
    if (lds)
        for (int b = t_; b < nq; b += kRsThreads) lut[b] = (V)qv[b];
    constexpr int64_t ld = kRsRanges + 1;
    unsigned bad = 0;
    const int tl = (w == 0 && lane < G) ? info->tlast1[lane] - 1 : -1;  // -1: an empty run
    int32_t nlo = 0, nhi = 0;
    auto fetch = [&](int64_t tt) {
        if (tl >= 0 && tt <= tl) {
            nlo = bounds[(int64_t)lane * ld + tt];
            nhi = bounds[(int64_t)lane * ld + tt + 1];
        }
    };
    // wave 0: range tt's run pieces into buffer b (lane g < G: run g), from bounds (clo, chi)
    auto plan = [&](int b, int64_t tt, int32_t clo, int32_t chi) {
        int64_t lo = 0, len = 0, before = 0;
        if (lane < G) {
            const int64_t s0 = S[lane], s1 = S[lane + 1];
            lo = s1;
            int64_t hi = s1;
            if (tl >= 0 && tt <= tl) {
                lo = clo;
                hi = chi;
            }
            before = lo - s0;
            len = hi - lo;
            lo_s[b][lane] = lo;
        }
        int64_t x = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane < kMaxGroups) pre[b][lane + 1] = (int32_t)x;
        if (lane == 0) pre[b][0] = 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) before += __shfl_xor(before, off, 64);
        if (lane == 0) obase[b] = before;
    };
    auto run_of = [&](int b, int j) -> int {
        if (G <= 8) {
            int g = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) g += (q + 1 <= G && pre[b][q + 1] <= j) ? 1 : 0;
            return g;
        }
        return agg_search32(pre[b], G, j);
    };
    auto load = [&](int b, int32_t (&kk)[kRsBatch], int32_t (&bb)[kRsBatch]) {
        const int cnt = pre[b][G];
        // the run ends in registers once per range (at most 8 runs), not one LDS read per run and element
        int32_t re[8];
#pragma unroll
        for (int q = 0; q < 8; q++) re[q] = q + 1 <= G ? pre[b][q + 1] : INT32_MAX;
#pragma unroll
        for (int u = 0; u < kRsBatch; u++) {
            const int j = u * kRsThreads + t_;
            kk[u] = -1;
            bb[u] = 0;
            if (j < cnt) {
                int g = 0;
                if (G <= 8) {
#pragma unroll
                    for (int q = 0; q < 8; q++) g += re[q] <= j ? 1 : 0;
                } else {
                    g = run_of(b, j);
                }
                const int64_t i = lo_s[b][g] + (j - pre[b][g]);
                kk[u] = gk[i];
                bb[u] = gb[i];
            }
        }
    };
    int32_t kc[kRsBatch], bc[kRsBatch], kn[kRsBatch], bn[kRsBatch];
    int buf = 0;
    const int64_t t0 = blockIdx.x;
    if (t0 <= tmax) {
        if (w == 0) {
            fetch(t0);
            plan(0, t0, nlo, nhi);
            fetch(t0 + gridDim.x);
        }
        __syncthreads();
        load(0, kc, bc);
    }
    for (int64_t t = t0; t <= tmax; t += gridDim.x) {
        const bool more = t + gridDim.x <= tmax;
        const int nbuf = buf == 2 ? 0 : buf + 1;
        if (w == 0 && more) {  // the next range's piece table, from the bounds fetched one range ago
            plan(nbuf, t + gridDim.x, nlo, nhi);
            fetch(t + 2 * (int64_t)gridDim.x);
        }
        bm[t_] = 0;
        __syncthreads();  // bm zeroed, the next plan visible, the previous emit done with bm / slot
        if (more) load(nbuf, kn, bn);  // in flight while this range is marked and emitted
        const int cnt = pre[buf][G];
        // pass 1: this range's keys into the bitmap, their bins into the offset slots
        auto to_slot = [&](int32_t b) -> ST {
            if constexpr (kBins) {
                return b;
            } else {
                if (b < 0 || b >= nq) {  // quantValues[bin] out of bounds: the rounds report it
                    bad = 1;
                    return 0;
                }
                return (ST)b;
            }
        };
#pragma unroll
        for (int u = 0; u < kRsBatch; u++) {
            if (kc[u] < 0) continue;
            const uint32_t off = (uint32_t)kc[u] & (kRsRange - 1), bit = 1u << (off & 31);
            if (atomicOr(&bm[off >> 5], bit) & bit) bad = 1;  // a repeated key
            slot[off] = to_slot(bc[u]);
        }
        for (int j = kRsThreads * kRsBatch + t_; j < cnt; j += kRsThreads) {  // past the registers
            const int g = run_of(buf, j);
            const int64_t i = lo_s[buf][g] + (j - pre[buf][g]);
            const int32_t k = gk[i];
            const uint32_t off = (uint32_t)k & (kRsRange - 1), bit = 1u << (off & 31);
            if (atomicOr(&bm[off >> 5], bit) & bit) bad = 1;
            slot[off] = to_slot(gb[i]);
        }
        __syncthreads();
        if (cnt > 0) {  // workgroup-uniform
            // pass 2: thread t_ owns bitmap word t_: its set bits go out in key order from its
            // exclusive popcount prefix
            const uint32_t word = bm[t_];
            const uint32_t own = __popc(word);
            uint32_t inc = own;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = __shfl_up(inc, off, 64);
                if (lane >= off) inc += y;
            }
            if (lane == 63) wsum[w] = inc;
            __syncthreads();
            uint32_t run = inc - own;
            for (int q = 0; q < w; q++) run += wsum[q];
            for (uint32_t m = word; m; m &= m - 1, run++) ord[run] = (uint16_t)(32 * t_ + __ffs(m) - 1);
            __syncthreads();
            const int64_t ob = obase[buf];
            const int32_t kbase = (int32_t)(t * kRsRange);
            for (int j = t_; j < cnt; j += kRsThreads) {
                const int off = ord[j];
                keys_out[ob + j] = kbase + off;
                out[ob + j] = rs_value<V>((int32_t)slot[off], lut, qv, nq, lds, bad);
            }
        }
        buf = nbuf;
#pragma unroll
        for (int u = 0; u < kRsBatch; u++) {
            kc[u] = kn[u];
            bc[u] = bn[u];
        }
    }
    if (bad) atomicOr(&info->irregular, 2u);
}

hipError_t launch_rs_merge(hipStream_t st, const int32_t* gk, const int32_t* gb, int64_t n, const SpGroups* gp,
                           int32_t* bounds, RsInfo* info, int32_t* keys_out, void* out, int vkind, const double* qv,
                           int nq, bool bounds_ready) {
    if (n <= 0) return hipSuccess;
    const int64_t bgrid = sp_tiles(sp_tiles(n, 16), kSpThreads);
#ifdef SKML_AB
    if (!bounds_ready)
        hipLaunchKernelGGL(k_rs_bounds, dim3((unsigned)bgrid), dim3(kSpThreads), 0, st, gk, n, gp, bounds, info);
#else
    (void)bgrid;
    if (!bounds_ready) return hipErrorInvalidValue;  // the key query writes the ranges' bounds
#endif
    // persistent workgroups over the key ranges up to the largest key (read on the device): as many
    // as are resident at once (4 per CU), fewer for small inputs
    const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(sp_tiles(n, 4096), 1), 1024);
    // the pipelined form unless SKML_FORM_RS_ROUNDS = 2 asks for the plain one-pass kernel
#define SKML_RS_LAUNCH(K)                                                                                         \
    do {                                                                                                          \
        if (vkind == 0)                                                                                           \
            hipLaunchKernelGGL(K<int32_t>, dim3(grid), dim3(kRsThreads), 0, st, gk, gb, gp, bounds, info, keys_out, \
                               static_cast<int32_t*>(out), qv, nq);                                              \
        else if (vkind == 1)                                                                                      \
            hipLaunchKernelGGL(K<float>, dim3(grid), dim3(kRsThreads), 0, st, gk, gb, gp, bounds, info, keys_out,  \
                               static_cast<float*>(out), qv, nq);                                                \
        else                                                                                                      \
            hipLaunchKernelGGL(K<double>, dim3(grid), dim3(kRsThreads), 0, st, gk, gb, gp, bounds, info, keys_out, \
                               static_cast<double*>(out), qv, nq);                                               \
    } while (0)
#ifdef SKML_AB
    if (form(SKML_FORM_RS_ROUNDS) == 2) SKML_RS_LAUNCH(k_rs_merge);
    else
#endif
#ifndef SKML_RS_NARROW
#define SKML_RS_NARROW 1  // A/B builds: 0 keeps 16-bit slots for every values restore
#endif
    if (SKML_RS_NARROW && vkind != 0 && nq >= 1 && nq <= 256) {
        // the grid is what the CUs hold of the narrow form (5-6 per CU), fewer for small inputs
        static const int res_f = resident_blocks(k_rs_merge_pf<float, true>, kRsThreads);
        static const int res_d = resident_blocks(k_rs_merge_pf<double, true>, kRsThreads);
        const int res = vkind == 1 ? res_f : res_d;
        const unsigned g2 = (unsigned)std::min<int64_t>(std::max<int64_t>(sp_tiles(n, 4096), 1), res > 0 ? res : 1024);
        if (vkind == 1)
            hipLaunchKernelGGL((k_rs_merge_pf<float, true>), dim3(g2), dim3(kRsThreads), 0, st, gk, gb, gp, bounds, info,
                               keys_out, static_cast<float*>(out), qv, nq);
        else
            hipLaunchKernelGGL((k_rs_merge_pf<double, true>), dim3(g2), dim3(kRsThreads), 0, st, gk, gb, gp, bounds, info,
                               keys_out, static_cast<double*>(out), qv, nq);
    } else {
        SKML_RS_LAUNCH(k_rs_merge_pf);
    }
#undef SKML_RS_LAUNCH
    return hipGetLastError();
}

// values[bins[i]] (SparseVectorCompressor.java:118-126) from the double quantValues LUT
// (Quantizer.getValues, times any timesBy factors): as fp32, or the doubles themselves.
template <typename T>
__global__ __launch_bounds__(kSpThreads) void k_bin_values(const int32_t* __restrict__ bins, int64_t n,
                                                           const double* __restrict__ qv, int B,
                                                           T* __restrict__ vals, unsigned* __restrict__ err) {
    __shared__ T lut[4096];
    const bool lds = B <= 4096;
    if (lds) {
        for (int b = threadIdx.x; b < B; b += kSpThreads) lut[b] = (T)qv[b];
        __syncthreads();
    }
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kSpThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSpThreads) {
        const int b = bins[i];
        const bool ok = b >= 0 && b < B;  // Java: quantValues[bin] out of bounds throws
        bad |= !ok;
        vals[i] = !ok ? (T)0 : lds ? lut[b] : (T)qv[b];
    }
    if (bad) atomicOr(err, 1u);
}

template <typename T>
hipError_t launch_bin_values_t(hipStream_t st, const int32_t* bins, int64_t n, const double* qvalues, int B, T* vals,
                               unsigned* err) {
    if (n <= 0) return hipSuccess;
    const int64_t grid = std::min<int64_t>(sp_tiles(n, kSpThreads * 4), 4096);
    hipLaunchKernelGGL(k_bin_values<T>, dim3((unsigned)grid), dim3(kSpThreads), 0, st, bins, n, qvalues, B, vals, err);
    return hipGetLastError();
}
hipError_t launch_bin_values(hipStream_t st, const int32_t* bins, int64_t n, const double* qvalues, int B,
                             float* vals, unsigned* err) {
    return launch_bin_values_t<float>(st, bins, n, qvalues, B, vals, err);
}
hipError_t launch_bin_values64(hipStream_t st, const int32_t* bins, int64_t n, const double* qvalues, int B,
                               double* vals, unsigned* err) {
    return launch_bin_values_t<double>(st, bins, n, qvalues, B, vals, err);
}

}  // namespace skml
