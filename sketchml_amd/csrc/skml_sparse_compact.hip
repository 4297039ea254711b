// skml_sparse_compact.hip -- CDNA4 (gfx950) kernels of the sparse codec: compaction
// (DenseDoubleGradient.toSparse) and the column scan of the tile sums.
//   k_compact        DenseDoubleGradient.toSparse (ml/gradient/DenseDoubleGradient.scala:64-89):
//                    single-pass stream compaction with decoupled look-back (ticketed tiles).
#include <algorithm>

#include "skml_device.hpp"
#include "skml_lowp.hpp"
#include "skml_sparse.h"
#include "skml_sparse_device.hpp"

namespace skml {

// A count the host may be polling in coherent host memory (ctx_host_word): a system-scope store,
// so it is not held in L2.  No release: the host only reads the value, and everything that reads
// the compaction's output runs later on the same stream.
__device__ __forceinline__ void put_count(int64_t* p, int64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

#ifndef SKML_LOOKBACK_ROWS
#define SKML_LOOKBACK_ROWS 1  // predecessors per look-back step = 64 x this (A/B builds vary it)
#endif
// Decoupled look-back of one wave: the sum of the counts of the tiles before `tile` (every lane
// gets it).  One step loads 64 x K predecessors' status words at once (K per lane, all in flight),
// then walks them nearest first, in rows of 64, to the nearest inclusive prefix.  The tiles in
// flight finish at about the same time, so the nearest prefix sits several hundred tiles back: at
// 64 per step that took a dozen dependent L2 round trips per tile.
template <int K>
__device__ __forceinline__ uint64_t lookback_excl(const uint64_t* status, int64_t tile, int lane) {
    uint64_t acc = 0;
    int64_t p = tile - 1;
    bool done = false;
    while (!done) {
        uint64_t sv[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int64_t idx = p - (int64_t)(k * 64 + lane);
            sv[k] = idx >= 0 ? ld_status(&status[idx]) : kStPre;  // before tile 0: prefix 0
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (!done) {  // (no break: sv stays in registers only while every index is static)
                const int64_t idx = p - (int64_t)(k * 64 + lane);
                while (__ballot((sv[k] & ~kStMask) == 0)) {
                    __builtin_amdgcn_s_sleep(1);
                    if ((sv[k] & ~kStMask) == 0) sv[k] = ld_status(&status[idx]);
                }
                const uint64_t pre = __ballot((sv[k] & ~kStMask) == kStPre);
                const int stop = pre ? __ffsll((unsigned long long)pre) - 1 : 63;
                acc += lane <= stop ? (sv[k] & kStMask) : 0;
                done = pre != 0;
            }
        }
        p -= 64 * K;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    return acc;
}

// =============================================================================================
// Compaction (decoupled look-back)
// =============================================================================================
// Each workgroup compacts one tile of values, all of it held in registers (fp32: 16,384 values,
// 16 float4 per thread, slab j of the tile = float4 j * 256 + t; fp64: 8,192 values, two double2
// per slab), so a tile keeps 64 KiB of loads in flight and takes one look-back.  Ranks follow index order: slab by slab, and within a slab
// by float4, from wave-level scans of 16-bit packed per-slab counts plus the waves' slab totals.
constexpr int kCompactStage = 4096;  // kept elements staged in LDS; denser tiles store directly

// Element traits: fp32 tiles of 16,384 (64 per thread, 16 float4 slabs), fp64 tiles of 8,192 (32
// per thread, 8 slabs of two double2): 64 KiB of loads in flight per tile either way.
// bf16 / fp16 tiles of 16,384 as well (8 slabs of one 16-byte load of 8 values: 32 KiB in flight).
// kPer: values per thread per slab; reg: a value as the tile holds it in registers (the 16 bits
// themselves for the 16-bit types, widened only when kept); val: the compacted values' type.
template <typename T> struct CompactT;
template <> struct CompactT<float> {
    static constexpr int kTile = kCompactTile, kPer = 4;
    typedef float reg;
    typedef float val;
    typedef float v2 __attribute__((ext_vector_type(4)));  // one slab = one 16-byte load
    // Maths.scala:8 EPS: |x| > 1e-8 in double; for a float x that is |x| > RD_f32(1e-8) on the
    // magnitude bits, NaN excluded (abs bits above +inf's): keep_f32_bits, skml_lowp.hpp.
    static __device__ __forceinline__ bool keep(float v) { return keep_f32_bits(__float_as_uint(v)); }
    static __device__ __forceinline__ float value(float v) { return v; }
    static __device__ __forceinline__ float load1(const float* __restrict__ x, int64_t i) { return x[i]; }
};
template <> struct CompactT<double> {
    static constexpr int kTile = kCompactTile / 2, kPer = 4;
    typedef double reg;
    typedef double val;
    typedef double v2 __attribute__((ext_vector_type(2)));  // one slab = two 16-byte loads
    static __device__ __forceinline__ bool keep(double v) {  // |x| > 1e-8, NaN excluded
        const uint64_t a = (uint64_t)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull;
        return a > 0x3E45798EE2308C3Aull && a <= 0x7FF0000000000000ull;
    }
    static __device__ __forceinline__ double value(double v) { return v; }
    static __device__ __forceinline__ double load1(const double* __restrict__ x, int64_t i) { return x[i]; }
};
// The 16-bit keep tests equal CompactT<float>::keep of the widened value for every pattern
// (skml_lowp.hpp, tests/sparse_lowp_check.cpp); widening is exact, so the kept values are the fp32
// compaction's of the widened buffer bit for bit.
template <> struct CompactT<bf16_t> {
    static constexpr int kTile = kCompactTile, kPer = 8;
    typedef uint16_t reg;
    typedef float val;
    typedef u32x4_v v2;  // one slab = one 16-byte load of 8 values
    static __device__ __forceinline__ bool keep(uint16_t h) { return keep_bf16_bits(h); }
    static __device__ __forceinline__ float value(uint16_t h) { return __uint_as_float(widen_bf16_bits(h)); }
    static __device__ __forceinline__ uint16_t load1(const bf16_t* __restrict__ x, int64_t i) { return x[i].bits; }
};
template <> struct CompactT<f16_t> {
    static constexpr int kTile = kCompactTile, kPer = 8;
    typedef uint16_t reg;
    typedef float val;
    typedef u32x4_v v2;
    static __device__ __forceinline__ bool keep(uint16_t h) { return keep_f16_bits(h); }
    static __device__ __forceinline__ float value(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
    static __device__ __forceinline__ uint16_t load1(const f16_t* __restrict__ x, int64_t i) { return x[i].bits; }
};
// the 8 values of one 16-byte load, in index order (low half of each word first)
__device__ __forceinline__ void cb_unpack8(const u32x4_v& w, uint16_t* f) {
    f[0] = (uint16_t)w.x, f[1] = (uint16_t)(w.x >> 16), f[2] = (uint16_t)w.y, f[3] = (uint16_t)(w.y >> 16);
    f[4] = (uint16_t)w.z, f[5] = (uint16_t)(w.z >> 16), f[6] = (uint16_t)w.w, f[7] = (uint16_t)(w.w >> 16);
}
template <typename T>
constexpr int compact_tile() { return CompactT<T>::kTile; }

template <typename T>
__global__ __launch_bounds__(kSpThreads) void k_compact(const T* __restrict__ x, int64_t dim,
                                                        int32_t* __restrict__ keys,
                                                        typename CompactT<T>::val* __restrict__ vals,
                                                        uint64_t* status, unsigned* ticket, int64_t ntiles,
                                                        int64_t* nnz_out) {
    constexpr int kTile = CompactT<T>::kTile, kE = CompactT<T>::kPer;
    constexpr int kSlabs = kTile / (kE * kSpThreads);  // kE elements per thread per slab
    static_assert(kSlabs % 4 == 0 && kSlabs * kE <= 64, "16-bit slab counts, 4 per u64, 64-bit keep mask");
    typedef typename CompactT<T>::v2 vec;
    typedef typename CompactT<T>::reg reg;
    __shared__ uint32_t wtot[kSpThreads / 64][kSlabs];  // per-wave kept counts of each slab
    __shared__ int64_t s_tile;
    __shared__ uint64_t s_excl;
    __shared__ int32_t stage_k[kCompactStage];
    __shared__ typename CompactT<T>::val stage_v[kCompactStage];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) s_tile = (int64_t)atomicAdd(ticket, 1u);
    __syncthreads();
    const int64_t tile = s_tile;
    const int64_t base = tile * kTile;
    const int64_t lim = dim - base;
    reg f[kSlabs][kE];  // slab j of the tile = elements kE * (j * 256 + t) .. + kE - 1
    if constexpr (is_lowp<T>::value) {
        if (lim >= kTile && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
            const vec* src = reinterpret_cast<const vec*>(x + base);
#pragma unroll
            for (int j = 0; j < kSlabs; j++) cb_unpack8(__builtin_nontemporal_load(src + j * kSpThreads + t), f[j]);
        } else {  // a partial tile, or a pointer with only its element's alignment
#pragma unroll
            for (int j = 0; j < kSlabs; j++) {
                const int64_t e0 = kE * ((int64_t)j * kSpThreads + t);
#pragma unroll
                for (int e = 0; e < kE; e++) f[j][e] = e0 + e < lim ? CompactT<T>::load1(x, base + e0 + e) : (reg)0;
            }
        }
    } else if (lim >= kTile && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const vec* src = reinterpret_cast<const vec*>(x + base);
        constexpr int kVec = 4 / (16 / (int)sizeof(T) >= 4 ? 4 : 16 / (int)sizeof(T));  // loads per slab
        constexpr int kPer = 4 / kVec;                                                 // elements per load
#pragma unroll
        for (int j = 0; j < kSlabs; j++)
#pragma unroll
            for (int u = 0; u < kVec; u++) {
                const vec v = __builtin_nontemporal_load(src + ((int64_t)j * kSpThreads + t) * kVec + u);
#pragma unroll
                for (int e = 0; e < kPer; e++) f[j][u * kPer + e] = v[e];
            }
    } else {
#pragma unroll
        for (int j = 0; j < kSlabs; j++) {
            const int64_t e0 = 4 * ((int64_t)j * kSpThreads + t);
#pragma unroll
            for (int e = 0; e < 4; e++) f[j][e] = e0 + e < lim ? x[base + e0 + e] : (T)0;
        }
    }
    uint64_t keep = 0;
#pragma unroll
    for (int j = 0; j < kSlabs; j++)
#pragma unroll
        for (int e = 0; e < kE; e++) keep |= CompactT<T>::keep(f[j][e]) ? (1ull << (kE * j + e)) : 0ull;
    // wave-inclusive scans of the per-slab counts, four 16-bit lanes per u64
    uint64_t P[kSlabs / 4];
#pragma unroll
    for (int k = 0; k < kSlabs / 4; k++) {
        uint64_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
            v |= (uint64_t)__popcll((keep >> (kE * (4 * k + q))) & ((1ull << kE) - 1)) << (16 * q);
        P[k] = v;
    }
    uint64_t own[kSlabs / 4];
#pragma unroll
    for (int k = 0; k < kSlabs / 4; k++) own[k] = P[k];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < kSlabs / 4; k++) {
            const uint64_t y = __shfl_up(P[k], off, 64);
            if (lane >= off) P[k] += y;
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int j = 0; j < kSlabs; j++) wtot[w][j] = (uint32_t)(P[j >> 2] >> (16 * (j & 3))) & 0xFFFFu;
    }
    __syncthreads();
    // slab totals, this wave's offset inside each slab, and the tile total
    uint32_t slab_pre[kSlabs];
    uint32_t tile_total = 0;
#pragma unroll
    for (int j = 0; j < kSlabs; j++) {
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int u = 0; u < kSpThreads / 64; u++) {
            const uint32_t c = wtot[u][j];
            before += u < w ? c : 0u;
            tot += c;
        }
        slab_pre[j] = tile_total + before;
        tile_total += tot;
    }
    if (t < 64) {  // wave 0: publish the aggregate, then look back
        uint64_t excl = 0;
        if (tile == 0) {
            if (lane == 0) st_status(&status[0], kStPre | tile_total);
        } else {
            if (lane == 0) st_status(&status[tile], kStAgg | tile_total);
            excl = lookback_excl<sizeof(T) == 8 ? 1 : 4>(status, tile, lane);  // rows the register budget allows
            if (lane == 0) st_status(&status[tile], kStPre | (excl + tile_total));
        }
        if (lane == 0) {
            s_excl = excl;
            if (tile == ntiles - 1) put_count(nnz_out, (int64_t)(excl + tile_total));
        }
    }
    __syncthreads();
    const int64_t out0 = (int64_t)s_excl;
    if (tile_total <= (uint32_t)kCompactStage) {  // the tile's output through LDS: coalesced stores
#pragma unroll
        for (int j = 0; j < kSlabs; j++) {
            const uint32_t incl = (uint32_t)(P[j >> 2] >> (16 * (j & 3))) & 0xFFFFu;
            const uint32_t mine = (uint32_t)(own[j >> 2] >> (16 * (j & 3))) & 0xFFFFu;
            uint32_t pos = slab_pre[j] + incl - mine;
            const int32_t e0 = (int32_t)(base + kE * ((int64_t)j * kSpThreads + t));
#pragma unroll
            for (int e = 0; e < kE; e++)
                if ((keep >> (kE * j + e)) & 1ull) {
                    stage_k[pos] = e0 + e;
                    stage_v[pos] = CompactT<T>::value(f[j][e]);
                    pos++;
                }
        }
        __syncthreads();
        for (uint32_t q = t; q < tile_total; q += kSpThreads) {
            keys[out0 + q] = stage_k[q];
            vals[out0 + q] = stage_v[q];
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kSlabs; j++) {
        const uint64_t incl = (P[j >> 2] >> (16 * (j & 3))) & 0xFFFFull;
        const uint64_t mine = (own[j >> 2] >> (16 * (j & 3))) & 0xFFFFull;
        int64_t pos = out0 + slab_pre[j] + (int64_t)(incl - mine);
        const int32_t e0 = (int32_t)(base + kE * ((int64_t)j * kSpThreads + t));
#pragma unroll
        for (int e = 0; e < kE; e++)
            if ((keep >> (kE * j + e)) & 1ull) {
                keys[pos] = e0 + e;
                vals[pos] = CompactT<T>::value(f[j][e]);
                pos++;
            }
    }
}

// fp32 / bf16 / fp16 compaction over big tiles: kCbSub sub-tiles of 8,192 values per workgroup, processed in
// turn (the next sub-tile's 32 KiB of loads in flight while the current one is ranked), their kept
// values and in-sub-tile offsets staged in LDS; one decoupled look-back per 65,536 values (a
// quarter of k_compact's: its prefix frontier, 64 tiles per look-back step, no longer trails the
// tiles' arrival), then coalesced stores.  A tile keeping more than kCbCap values re-reads its
// input and stores directly.  A 16-bit sub-tile is 4 slabs of one 16-byte load of 8 values per
// thread (16 KiB in flight), held as the 16 bits and widened when staged or stored.
constexpr int kCbSubElems = 32 * kSpThreads;  // 8,192 values: 32 per thread
constexpr int kCbSub = 8, kCbTile = kCbSub * kCbSubElems, kCbCap = 8192;
template <typename X>
constexpr int cb_slabs() { return kCbSubElems / (CompactT<X>::kPer * kSpThreads); }  // fp32: 8 float4 slabs
static_assert(cb_slabs<float>() % 4 == 0 && cb_slabs<bf16_t>() % 4 == 0, "16-bit slab counts, 4 per u64");

// keep mask and in-sub-tile ranks of one sub-tile held as f[kCbSlabs][kE] (slab j = 16-byte load j * 256 + t)
template <int kCbSlabs>
struct CbRanks {
    uint32_t keep;
    uint32_t slab_pre[kCbSlabs];  // exclusive start of this thread's kept values of slab j in the sub-tile
    uint32_t total;               // kept values in the sub-tile
};
template <typename X, int kCbSlabs = cb_slabs<X>(), int kE = CompactT<X>::kPer>
__device__ __forceinline__ void cb_rank(const typename CompactT<X>::reg (&f)[kCbSlabs][kE],
                                        uint32_t (*wtot)[kCbSlabs], CbRanks<kCbSlabs>& R) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t keep = 0;
#pragma unroll
    for (int j = 0; j < kCbSlabs; j++)
#pragma unroll
        for (int e = 0; e < kE; e++) keep |= CompactT<X>::keep(f[j][e]) ? (1u << (kE * j + e)) : 0u;
    constexpr int kW = kCbSlabs / 4;
    uint64_t P[kW], own[kW];
#pragma unroll
    for (int k = 0; k < kW; k++) {
        uint64_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) v |= (uint64_t)__popc((keep >> (kE * (4 * k + q))) & ((1u << kE) - 1u)) << (16 * q);
        P[k] = own[k] = v;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < kW; k++) {
            const uint64_t y = __shfl_up(P[k], off, 64);
            if (lane >= off) P[k] += y;
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int j = 0; j < kCbSlabs; j++) wtot[w][j] = (uint32_t)(P[j >> 2] >> (16 * (j & 3))) & 0xFFFFu;
    }
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int j = 0; j < kCbSlabs; j++) {
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int u = 0; u < kSpThreads / 64; u++) {
            const uint32_t c = wtot[u][j];
            before += u < w ? c : 0u;
            tot += c;
        }
        const uint32_t incl = (uint32_t)(P[j >> 2] >> (16 * (j & 3))) & 0xFFFFu;
        const uint32_t mine = (uint32_t)(own[j >> 2] >> (16 * (j & 3))) & 0xFFFFu;
        R.slab_pre[j] = total + before + incl - mine;
        total += tot;
    }
    R.keep = keep;
    R.total = total;
    __syncthreads();  // wtot is reused by the next sub-tile
}

template <typename X, int kCbSlabs = cb_slabs<X>(), int kE = CompactT<X>::kPer>
__device__ __forceinline__ void cb_load(const X* __restrict__ x, int64_t base, int64_t dim,
                                        typename CompactT<X>::reg (&f)[kCbSlabs][kE]) {
    const int t = threadIdx.x;
    if constexpr (is_lowp<X>::value) {
        if (base + kCbSubElems <= dim) {  // x is 16-byte aligned (the launcher checks), base a multiple of 8
            const u32x4_v* src = reinterpret_cast<const u32x4_v*>(x + base);
#pragma unroll
            for (int j = 0; j < kCbSlabs; j++) cb_unpack8(__builtin_nontemporal_load(src + j * kSpThreads + t), f[j]);
        } else {
#pragma unroll
            for (int j = 0; j < kCbSlabs; j++) {
                const int64_t e0 = base + kE * ((int64_t)j * kSpThreads + t);
#pragma unroll
                for (int e = 0; e < kE; e++) f[j][e] = e0 + e < dim ? CompactT<X>::load1(x, e0 + e) : (uint16_t)0;
            }
        }
    } else if (base + kCbSubElems <= dim) {
        typedef float vec4 __attribute__((ext_vector_type(4)));
        const vec4* src = reinterpret_cast<const vec4*>(x + base);
#pragma unroll
        for (int j = 0; j < kCbSlabs; j++) {
            const vec4 v = __builtin_nontemporal_load(src + j * kSpThreads + t);
            f[j][0] = v[0], f[j][1] = v[1], f[j][2] = v[2], f[j][3] = v[3];
        }
    } else {
#pragma unroll
        for (int j = 0; j < kCbSlabs; j++) {
            const int64_t e0 = base + 4 * ((int64_t)j * kSpThreads + t);
#pragma unroll
            for (int e = 0; e < 4; e++) f[j][e] = e0 + e < dim ? x[e0 + e] : 0.0f;
        }
    }
}

#ifndef SKML_COMPACT_PERSIST
#define SKML_COMPACT_PERSIST 0  // 1: the persistent form (A/B builds)
#endif
// One tile per workgroup.  The persistent form (SKML_COMPACT_PERSIST 1, A/B builds) takes the next
// tile's ticket before its look-back and loads that tile's first sub-tile while its stores drain,
// with the grid at what the CUs hold at once (tickets are taken in order by running workgroups and
// a workgroup waits only on lower tickets, so the look-back always progresses); it measured 10-20
// us slower per C3 encode (profiles/ab/r06_compact_persist.txt).
template <typename X>
__global__ __launch_bounds__(kSpThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_compact_big(const X* __restrict__ x, int64_t dim,
                                                            int32_t* __restrict__ keys, float* __restrict__ vals,
                                                            uint64_t* status, unsigned* ticket, int64_t ntiles,
                                                            int64_t* nnz_out) {
    __shared__ float st_v[kCbCap];
    __shared__ uint16_t st_k[kCbCap];  // offset inside the sub-tile (< 2^14)
    constexpr int kCbSlabs = cb_slabs<X>(), kE = CompactT<X>::kPer;
    typedef typename CompactT<X>::reg reg;
    __shared__ uint32_t wtot[kSpThreads / 64][kCbSlabs];
    __shared__ uint32_t sub_pre[kCbSub + 1];
    __shared__ int64_t s_tile;
    __shared__ uint64_t s_excl;
    const int t = threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) __builtin_trap();  // the launcher checks alignment
    if (t == 0) s_tile = (int64_t)atomicAdd(ticket, 1u);
    __syncthreads();
    int64_t tile = s_tile;
    if (tile >= ntiles) return;  // workgroup-uniform
    reg f[kCbSlabs][kE], g[kCbSlabs][kE];
    cb_load(x, tile * kCbTile, dim, f);
#pragma unroll 1
    while (true) {
        const int64_t base = tile * kCbTile;
        uint32_t run = 0;
#pragma unroll 1
        for (int sb = 0; sb < kCbSub; sb++) {
            reg (&cur)[kCbSlabs][kE] = f;
            if (sb + 1 < kCbSub) cb_load(x, base + (int64_t)(sb + 1) * kCbSubElems, dim, g);
            CbRanks<kCbSlabs> R;
            cb_rank<X>(cur, wtot, R);
            if (t == 0) sub_pre[sb] = run;
            if (run + R.total <= (uint32_t)kCbCap) {
#pragma unroll
                for (int j = 0; j < kCbSlabs; j++) {
                    uint32_t pos = run + R.slab_pre[j];
                    const int off0 = kE * (j * kSpThreads + t);
#pragma unroll
                    for (int e = 0; e < kE; e++)
                        if ((R.keep >> (kE * j + e)) & 1u) {
                            st_v[pos] = CompactT<X>::value(cur[j][e]);
                            st_k[pos] = (uint16_t)(off0 + e);
                            pos++;
                        }
                }
            }
            run += R.total;
#pragma unroll
            for (int j = 0; j < kCbSlabs; j++)
#pragma unroll
                for (int e = 0; e < kE; e++) f[j][e] = g[j][e];
        }
        const uint32_t tile_total = run;
        // every thread read s_tile before cb_rank's barriers: the next ticket may land there now
        if (SKML_COMPACT_PERSIST && t == 0) s_tile = (int64_t)atomicAdd(ticket, 1u);
        if (t < 64) {  // wave 0: publish the aggregate, then look back
            const int lane = t;
            uint64_t excl = 0;
            if (tile == 0) {
                if (lane == 0) st_status(&status[0], kStPre | tile_total);
            } else {
                if (lane == 0) st_status(&status[tile], kStAgg | tile_total);
                excl = lookback_excl<SKML_LOOKBACK_ROWS>(status, tile, lane);
                if (lane == 0) st_status(&status[tile], kStPre | (excl + tile_total));
            }
            if (lane == 0) {
                s_excl = excl;
                sub_pre[kCbSub] = tile_total;
                if (tile == ntiles - 1) put_count(nnz_out, (int64_t)(excl + tile_total));
            }
        }
        __syncthreads();
        const int64_t out0 = (int64_t)s_excl;
        const int64_t next = SKML_COMPACT_PERSIST ? s_tile : ntiles;
        if (tile_total <= (uint32_t)kCbCap) {
            if (next < ntiles) cb_load(x, next * kCbTile, dim, f);  // in flight while this tile's stores drain
            for (uint32_t q = t; q < tile_total; q += kSpThreads) {
                int sb = 0;
#pragma unroll
                for (int k = 1; k < kCbSub; k++) sb += q >= sub_pre[k] ? 1 : 0;
                keys[out0 + q] = (int32_t)(base + (int64_t)sb * kCbSubElems + st_k[q]);
                vals[out0 + q] = st_v[q];
            }
        } else {
            // more kept values than the stage holds: read each sub-tile again and store directly
            for (int sb = 0; sb < kCbSub; sb++) {
                const int64_t sbase = base + (int64_t)sb * kCbSubElems;
                cb_load(x, sbase, dim, f);
                CbRanks<kCbSlabs> R;
                cb_rank<X>(f, wtot, R);
#pragma unroll
                for (int j = 0; j < kCbSlabs; j++) {
                    int64_t pos = out0 + sub_pre[sb] + R.slab_pre[j];
                    const int64_t e0 = sbase + kE * ((int64_t)j * kSpThreads + t);
#pragma unroll
                    for (int e = 0; e < kE; e++)
                        if ((R.keep >> (kE * j + e)) & 1u) {
                            keys[pos] = (int32_t)(e0 + e);
                            vals[pos] = CompactT<X>::value(f[j][e]);
                            pos++;
                        }
                }
            }
            if (next < ntiles) cb_load(x, next * kCbTile, dim, f);
        }
        if (next >= ntiles) break;
        __syncthreads();  // the stage, sub_pre and s_excl are the next tile's
        tile = next;
    }
}

template <typename T>
hipError_t launch_compact_t(hipStream_t st, const T* x, int64_t dim, int32_t* keys, typename CompactT<T>::val* vals,
                            uint64_t* status, unsigned* ticket, int64_t* nnz_out) {
    const int64_t tiles = sp_tiles(dim, compact_tile<T>());
    if (tiles <= 0) return hipMemsetAsync(nnz_out, 0, sizeof(int64_t), st);
    hipLaunchKernelGGL(k_compact<T>, dim3((unsigned)tiles), dim3(kSpThreads), 0, st, x, dim, keys, vals, status,
                       ticket, tiles, nnz_out);
    return hipGetLastError();
}
// fp32, bf16 and fp16 input, fp32 values out
template <typename X>
hipError_t launch_compact_x(hipStream_t st, const X* x, int64_t dim, int32_t* keys, float* vals, uint64_t* status,
                            unsigned* ticket, int64_t* nnz_out) {
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0 || dim < kCbTile)  // small or unaligned: the one-tile kernel
        return launch_compact_t<X>(st, x, dim, keys, vals, status, ticket, nnz_out);
    const int64_t tiles = sp_tiles(dim, kCbTile);
    int64_t grid = tiles;
    if (SKML_COMPACT_PERSIST) {  // the workgroups the CUs hold at once
        static const int resident = resident_blocks(k_compact_big<X>, kSpThreads);
        if (resident > 0) grid = std::min<int64_t>(tiles, resident);
    }
    hipLaunchKernelGGL(k_compact_big<X>, dim3((unsigned)grid), dim3(kSpThreads), 0, st, x, dim, keys, vals, status,
                       ticket, tiles, nnz_out);
    return hipGetLastError();
}
hipError_t launch_compact(hipStream_t st, const float* x, int64_t dim, int32_t* keys, float* vals,
                          uint64_t* status, unsigned* ticket, int64_t* nnz_out) {
    return launch_compact_x<float>(st, x, dim, keys, vals, status, ticket, nnz_out);
}
hipError_t launch_compact(hipStream_t st, const bf16_t* x, int64_t dim, int32_t* keys, float* vals,
                          uint64_t* status, unsigned* ticket, int64_t* nnz_out) {
    return launch_compact_x<bf16_t>(st, x, dim, keys, vals, status, ticket, nnz_out);
}
hipError_t launch_compact(hipStream_t st, const f16_t* x, int64_t dim, int32_t* keys, float* vals,
                          uint64_t* status, unsigned* ticket, int64_t* nnz_out) {
    return launch_compact_x<f16_t>(st, x, dim, keys, vals, status, ticket, nnz_out);
}
hipError_t launch_compact64(hipStream_t st, const double* x, int64_t dim, int32_t* keys, double* vals,
                            uint64_t* status, unsigned* ticket, int64_t* nnz_out) {
    return launch_compact_t<double>(st, x, dim, keys, vals, status, ticket, nnz_out);
}

// =============================================================================================
// Column scan of [tiles][K] u64 tile sums (one workgroup per column)
// =============================================================================================
// One workgroup of 1,024 threads per column, 8K entries per pass.  A 1,024-thread workgroup needs
// 16 wave slots of one CU at once, and in Gradient.sum it waits for a CU beside the other
// restore's k_dec_keys (profiles/r06c_aggregate_timeline.txt); 256-thread one-pass scans remove
// that wait but ran slower end to end (restore +13 us, Gradient.sum +80 us: the two restores'
// key queries then overlap each other, profiles/ab/r06_scan_threads.txt).
#ifndef SKML_SCAN_THREADS
#define SKML_SCAN_THREADS 1024  // A/B builds: 256 (with SKML_SCAN_PER 64)
#endif
#ifndef SKML_SCAN_PER
#define SKML_SCAN_PER 8
#endif
constexpr int kScanThreads = SKML_SCAN_THREADS, kScanPer = SKML_SCAN_PER;
static_assert(kScanPer % 2 == 0, "16-byte loads of two entries");
// Entry (i, k) at sums[k * ld + i * es]: [tiles][K] row-major (ld 1, es K) or one column of
// tiles + 1 entries per k (ld tiles + 1, es 1: contiguous column reads).
// THREADS x PER entries per pass (kScanThreads x kScanPer by default; the sparse encode's side
// chain takes 256-thread workgroups, launch_scan_cols_small)
template <int THREADS = kScanThreads, int PER = kScanPer>
__global__ __launch_bounds__(THREADS) void k_scan_cols(uint64_t* sums, int64_t tiles, int64_t ld, int64_t es) {
    constexpr int kScanThreads = THREADS, kScanPer = PER;
    __shared__ uint64_t sh[kScanThreads / 64];
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint64_t carry = 0;
    for (int64_t c0 = 0; c0 < tiles; c0 += kScanThreads * kScanPer) {
        uint64_t loc[kScanPer], s = 0;
        const int64_t i0 = c0 + t * kScanPer;
        if (es == 1 && i0 + kScanPer <= tiles && ((k * ld + i0) & 1) == 0) {  // 16-byte loads
            typedef uint64_t u64x2_t __attribute__((ext_vector_type(2)));
            const u64x2_t* src = reinterpret_cast<const u64x2_t*>(sums + k * ld + i0);
#pragma unroll
            for (int j = 0; j < kScanPer / 2; j++) {
                const u64x2_t v = src[j];
                loc[2 * j] = v.x;
                loc[2 * j + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kScanPer; j++) {
                const int64_t i = i0 + j;
                loc[j] = i < tiles ? sums[k * ld + i * es] : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < kScanPer; j++) s += loc[j];
        const uint64_t inc = wave_incl_u64(s, lane);
        if (lane == 63) sh[w] = inc;
        __syncthreads();
        uint64_t before = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < kScanThreads / 64; j++) {
            const uint64_t x = sh[j];
            before += j < w ? x : 0;
            tot += x;
        }
        __syncthreads();
        uint64_t run = carry + before + inc - s;
#pragma unroll
        for (int j = 0; j < kScanPer; j++) {
            const int64_t i = c0 + t * kScanPer + j;
            if (i < tiles) sums[k * ld + i * es] = run;
            run += loc[j];
        }
        carry += tot;
    }
    if (t == 0) sums[k * ld + tiles * es] = carry;
}

hipError_t launch_scan_cols(hipStream_t st, uint64_t* sums, int64_t tiles, int K) {
    hipLaunchKernelGGL(k_scan_cols<>, dim3(K), dim3(kScanThreads), 0, st, sums, tiles, (int64_t)1, (int64_t)K);
    return hipGetLastError();
}
hipError_t launch_scan_cols_major(hipStream_t st, uint64_t* sums, int64_t tiles, int K) {
    hipLaunchKernelGGL(k_scan_cols<>, dim3(K), dim3(kScanThreads), 0, st, sums, tiles, tiles + 1, (int64_t)1);
    return hipGetLastError();
}
// The same scan on 256-thread workgroups: in the sparse encode's side chain a 1,024-thread
// workgroup waits for a whole CU's wave slots beside the MinMax scatter (4-5 us alone, 57-70 us
// there), which pushed the DeltaAdaptive writer onto the bucket minima.
hipError_t launch_scan_cols_small(hipStream_t st, uint64_t* sums, int64_t tiles, int K) {
    hipLaunchKernelGGL((k_scan_cols<256, 32>), dim3(K), dim3(256), 0, st, sums, tiles, (int64_t)1, (int64_t)K);
    return hipGetLastError();
}

}  // namespace skml
