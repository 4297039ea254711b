// skml_sparse_partition.hip -- CDNA4 (gfx950) kernels of the sparse codec: group partition and the
// device-side encode plan.
//   k_part_*         FSketchUtils.partition (frequency/FSketchUtils.java:30-47): stable counting
//                    sort of (key, bin) by group, group = #{edges <= bin}.
//   k_sp_plan_*      the per-group decisions of the encode (group edges and shapes, interval
//                    choice), one workgroup each, no host round trip.
#include <algorithm>

#include "skml_device.hpp"
#include "skml_sparse.h"
#include "skml_sparse_device.hpp"

namespace skml {

// =============================================================================================
// Partition by group (stable)
// =============================================================================================
// packed code of element e (LSB-first codes, code_bits in {1,2,4,8,16})
__device__ __forceinline__ int32_t code_at(const uint8_t* codes, int64_t e, int bits) {
    switch (bits) {
        case 8: return codes[e];
        case 16: return reinterpret_cast<const uint16_t*>(codes)[e];
        case 4: return (codes[e >> 1] >> ((e & 1) * 4)) & 15;
        case 2: return (codes[e >> 2] >> ((e & 3) * 2)) & 3;
        default: return (codes[e >> 3] >> (e & 7)) & 1;
    }
}

// #{edges[j] <= bin} over a sorted 64-entry LDS table padded with INT32_MAX
__device__ __forceinline__ int group_of_bin(const int32_t* E, int32_t bin) {
    int g = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1)
        if (E[g + step - 1] <= bin) g += step;
    return g;
}

__device__ __forceinline__ void load_edges(const SpGroups* gp, int32_t* E) {
    for (int j = threadIdx.x; j < kMaxGroups; j += blockDim.x) E[j] = j < gp->G ? gp->edges[j] : INT32_MAX;
}

// Up to kFewGroups groups (the default is 8): the edges sit in registers, the group of a bin is a
// sum of compares, and the per-group counts are 8-bit fields of one u64 per lane (at most 8
// elements per lane and step), reduced across the wave as two u64 of 16-bit fields.
constexpr int kFewGroups = 8;
struct FewEdges {
    int32_t e[kFewGroups - 1];  // edges[0 .. G-2], INT32_MAX beyond (edges[G-1] = binNum is above every bin)
};
__device__ __forceinline__ FewEdges few_edges(const SpGroups* gp, int G) {
    FewEdges f;
#pragma unroll
    for (int j = 0; j < kFewGroups - 1; j++) f.e[j] = j < G - 1 ? gp->edges[j] : INT32_MAX;
    return f;
}
__device__ __forceinline__ int few_group(const FewEdges& f, int32_t bin) {
    int g = 0;
#pragma unroll
    for (int j = 0; j < kFewGroups - 1; j++) g += f.e[j] <= bin ? 1 : 0;
    return g;
}
// wave sums of the 8-bit fields of acc, as 16-bit fields: groups 0,2,4,6 in lo and 1,3,5,7 in hi
__device__ __forceinline__ void few_wave_sum(uint64_t acc, uint64_t& lo, uint64_t& hi) {
    lo = acc & 0x00FF00FF00FF00FFull;
    hi = (acc >> 8) & 0x00FF00FF00FF00FFull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo += __shfl_xor(lo, off, 64);
        hi += __shfl_xor(hi, off, 64);
    }
}
__device__ __forceinline__ uint32_t few_field(uint64_t lo, uint64_t hi, int g) {
    return (uint32_t)(((g & 1) ? hi : lo) >> (16 * (g >> 1))) & 0xFFFFu;
}

// kPartTiles consecutive tiles per workgroup, their code loads issued together (one tile per
// workgroup left the 2 KB-per-workgroup pass bound by workgroup dispatch: 26 us at C3).
constexpr int kPartTiles = 4;
__global__ __launch_bounds__(kSpThreads) void k_part_count(const uint8_t* __restrict__ qpayload, int64_t n,
                                                           const SpGroups* __restrict__ gp,
                                                           uint64_t* __restrict__ tile_counts,
                                                           uint32_t* __restrict__ z32, int64_t n32,
                                                           uint64_t* __restrict__ z64, int64_t n64) {
    for (int64_t z = (int64_t)blockIdx.x * kSpThreads + threadIdx.x, step = (int64_t)gridDim.x * kSpThreads;
         z < n32 || z < n64; z += step) {
        if (z < n32) z32[z] = 0;
        if (z < n64) z64[z] = 0;
    }
    if (gp->status) return;
    __shared__ int32_t E[kMaxGroups];
    __shared__ uint32_t cnt[kPartTiles][kMaxGroups];
    __shared__ uint64_t wsum[kPartTiles][kSpThreads / 64][2];
    const skml_dense_header* h = reinterpret_cast<const skml_dense_header*>(qpayload);
    const uint8_t* codes = qpayload + h->codes_offset;
    const int bits = h->code_bits, G = gp->G;
    const int64_t tiles = (n + kSpTile - 1) / kSpTile;
    const int64_t tile0 = (int64_t)blockIdx.x * kPartTiles;
    const int t = threadIdx.x;
    if (G <= kFewGroups) {  // 8 consecutive elements per lane, counted in registers
        static_assert(kSpTile == 8 * kSpThreads, "one 8-element run per lane");
        const FewEdges fe = few_edges(gp, G);
        const bool fast = bits == 8 && ((reinterpret_cast<uintptr_t>(codes) & 7) == 0);
        uint64_t w8[kPartTiles];
#pragma unroll
        for (int k = 0; k < kPartTiles; k++) {
            const int64_t i0 = (tile0 + k) * kSpTile + 8 * t;
            w8[k] = fast && i0 + 8 <= n ? *reinterpret_cast<const uint64_t*>(codes + i0) : 0ull;
        }
#pragma unroll
        for (int k = 0; k < kPartTiles; k++) {
            const int64_t i0 = (tile0 + k) * kSpTile + 8 * t;
            uint64_t acc = 0;
            if (fast && i0 + 8 <= n) {
#pragma unroll
                for (int e = 0; e < 8; e++) acc += 1ull << (8 * few_group(fe, (int32_t)((w8[k] >> (8 * e)) & 255u)));
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (i0 + e < n) acc += 1ull << (8 * few_group(fe, code_at(codes, i0 + e, bits)));
            }
            uint64_t lo, hi;
            few_wave_sum(acc, lo, hi);
            if ((t & 63) == 0) {
                wsum[k][t >> 6][0] = lo;
                wsum[k][t >> 6][1] = hi;
            }
        }
        __syncthreads();
        if (t < kPartTiles * G) {
            const int k = t / G, g = t - k * G;
            if (tile0 + k < tiles) {
                uint32_t c = 0;
#pragma unroll
                for (int w = 0; w < kSpThreads / 64; w++) c += few_field(wsum[k][w][0], wsum[k][w][1], g);
                tile_counts[(int64_t)g * (tiles + 1) + tile0 + k] = c;
            }
        }
        return;
    }
    load_edges(gp, E);
    for (int j = t; j < kPartTiles * kMaxGroups; j += kSpThreads) cnt[j / kMaxGroups][j % kMaxGroups] = 0;
    __syncthreads();
    for (int k = 0; k < kPartTiles; k++)
        for (int j = t; j < kSpTile; j += kSpThreads) {
            const int64_t i = (tile0 + k) * kSpTile + j;
            if (i < n) atomicAdd(&cnt[k][group_of_bin(E, code_at(codes, i, bits))], 1u);
        }
    __syncthreads();
    for (int j = t; j < kPartTiles * G; j += kSpThreads) {
        const int k = j / G, g = j - k * G;
        if (tile0 + k < tiles) tile_counts[(int64_t)g * (tiles + 1) + tile0 + k] = cnt[k][g];
    }
}

hipError_t launch_part_count(hipStream_t st, const void* qpayload, int64_t n, const SpGroups* gp,
                             uint64_t* tile_counts, uint32_t* z32, int64_t n32, uint64_t* z64, int64_t n64) {
    const int64_t tiles = sp_tiles(n, kSpTile);
    if (tiles <= 0) {
        if (n32 > 0) {
            hipError_t e = hipMemsetAsync(z32, 0, sizeof(uint32_t) * (size_t)n32, st);
            if (e != hipSuccess) return e;
        }
        return n64 > 0 ? hipMemsetAsync(z64, 0, sizeof(uint64_t) * (size_t)n64, st) : hipSuccess;
    }
    hipLaunchKernelGGL(k_part_count, dim3((unsigned)((tiles + kPartTiles - 1) / kPartTiles)), dim3(kSpThreads), 0, st,
                       reinterpret_cast<const uint8_t*>(qpayload), n, gp, tile_counts, z32, n32, z64, n64);
    return hipGetLastError();
}

// Wave w of the tile owns elements [w*512, (w+1)*512), 64 per step in order; lanes with the same
// group are ranked by lane (peer mask from log2(G) ballots), so the scatter is stable.  The tile
// is first laid out in group order in LDS, then each group's run is stored with consecutive lanes
// on consecutive output indices (direct per-lane stores split every step into G short segments).
__global__ __launch_bounds__(kSpThreads) void k_part_scatter(const int32_t* __restrict__ keys,
                                                             const uint8_t* __restrict__ qpayload, int64_t n,
                                                             const SpGroups* __restrict__ gp,
                                                             const uint64_t* __restrict__ tile_base,
                                                             int32_t* __restrict__ gkeys, uint16_t* __restrict__ gbins,
                                                             int runs) {
    if (gp->status) return;
    constexpr int kWaves = kSpThreads / 64, kSteps = kSpTile / kSpThreads;
    __shared__ int32_t E[kMaxGroups];
    __shared__ int64_t wb[kWaves][kMaxGroups];  // counts, then running LDS slot per (wave, group)
    __shared__ int64_t gdst[kMaxGroups];        // output index of a group's slot 0 in the tile
    __shared__ int32_t sk[kSpTile], sb[kSpTile];
    __shared__ uint8_t sg[kSpTile];
    const skml_dense_header* h = reinterpret_cast<const skml_dense_header*>(qpayload);
    const uint8_t* codes = qpayload + h->codes_offset;
    const int bits = h->code_bits, G = gp->G;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const bool few = G <= kFewGroups;
    // the output base of group t's run in this tile, read before the counting (no round trip later)
    int64_t gbase = 0;
    if (t < G) gbase = gp->gstart[t] + (int64_t)tile_base[(int64_t)t * ((int64_t)gridDim.x + 1) + blockIdx.x];
    if (few && runs) {
        // Thread t owns the tile's elements [8t, 8t + 8): one 32-byte key load and one 8-byte code
        // load per thread.  Stable ranks without ballots: the thread's per-group counts packed as
        // 16-bit fields (groups 0,2,4,6 in lo, 1,3,5,7 in hi), a wave scan of the packed words,
        // the waves' totals through LDS.
        const FewEdges fe = few_edges(gp, G);
        const int64_t i0 = (int64_t)blockIdx.x * kSpTile + 8 * t;
        int32_t kk[8], bb[8], gg[8];
        const bool full = i0 + 8 <= n;
        if (full && (reinterpret_cast<uintptr_t>(keys + i0) & 15) == 0) {
            const int4 a = *reinterpret_cast<const int4*>(keys + i0), b = *reinterpret_cast<const int4*>(keys + i0 + 4);
            kk[0] = a.x, kk[1] = a.y, kk[2] = a.z, kk[3] = a.w, kk[4] = b.x, kk[5] = b.y, kk[6] = b.z, kk[7] = b.w;
        } else {
#pragma unroll
            for (int s = 0; s < 8; s++) kk[s] = i0 + s < n ? keys[i0 + s] : 0;
        }
        if (full && bits == 8 && (reinterpret_cast<uintptr_t>(codes + i0) & 7) == 0) {
            const uint64_t w8 = *reinterpret_cast<const uint64_t*>(codes + i0);
#pragma unroll
            for (int s = 0; s < 8; s++) bb[s] = (int32_t)((w8 >> (8 * s)) & 255u);
        } else {
#pragma unroll
            for (int s = 0; s < 8; s++) bb[s] = i0 + s < n ? code_at(codes, i0 + s, bits) : 0;
        }
        uint64_t lo = 0, hi = 0;  // this thread's per-group counts
#pragma unroll
        for (int s = 0; s < 8; s++) {
            gg[s] = i0 + s < n ? few_group(fe, bb[s]) : -1;
            if (gg[s] >= 0) {
                const uint64_t one = 1ull << (16 * (gg[s] >> 1));
                if (gg[s] & 1) hi += one;
                else lo += one;
            }
        }
        uint64_t li = lo, hi_i = hi;  // inclusive wave scans
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t yl = __shfl_up(li, off, 64), yh = __shfl_up(hi_i, off, 64);
            if (lane >= off) {
                li += yl;
                hi_i += yh;
            }
        }
        __shared__ uint64_t wt[kWaves][2];
        __shared__ int32_t wbase[kWaves][kFewGroups];  // LDS slot of (wave, group)'s first element
        if (lane == 63) {
            wt[w][0] = li;
            wt[w][1] = hi_i;
        }
        __syncthreads();
        if (t < 64) {  // lane g < G: the tile's group g totals, the LDS layout in group order
            uint32_t c = 0;
            if (lane < G)
                for (int j = 0; j < kWaves; j++) c += few_field(wt[j][0], wt[j][1], lane);
            uint32_t x = c;  // inclusive scan over the groups
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = __shfl_up(x, off, 64);
                if (lane >= off) x += y;
            }
            if (lane < G) {
                uint32_t run = x - c;
                gdst[lane] = gbase - (int64_t)run;
                for (int j = 0; j < kWaves; j++) {
                    wbase[j][lane] = (int32_t)run;
                    run += few_field(wt[j][0], wt[j][1], lane);
                }
            }
        }
        __syncthreads();
        const uint64_t le = li - lo, he = hi_i - hi;  // exclusive: earlier lanes of this wave
        uint64_t seen_l = 0, seen_h = 0;              // this thread's earlier elements
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int g = gg[s];
            if (g < 0) continue;
            const int pos = wbase[w][g] + (int)few_field(le, he, g) + (int)few_field(seen_l, seen_h, g);
            sk[pos] = kk[s];
            sb[pos] = bb[s];
            sg[pos] = (uint8_t)g;
            const uint64_t one = 1ull << (16 * (g >> 1));
            if (g & 1) seen_h += one;
            else seen_l += one;
        }
        __syncthreads();
        const int tile_n = (int)std::min<int64_t>(kSpTile, n - (int64_t)blockIdx.x * kSpTile);
        for (int q = t; q < tile_n; q += kSpThreads) {
            const int64_t dst = gdst[sg[q]] + q;
            gkeys[dst] = sk[q];
            gbins[dst] = (uint16_t)sb[q];
        }
        return;
    }
    if (!few) {
        load_edges(gp, E);
        for (int j = t; j < kWaves * kMaxGroups; j += kSpThreads) wb[j / kMaxGroups][j % kMaxGroups] = 0;
        __syncthreads();
    }
    const int64_t base = (int64_t)blockIdx.x * kSpTile + (int64_t)w * (kSpTile / kWaves);
    int32_t kk[kSteps], gg[kSteps], bb[kSteps];
    if (few) {  // the wave's group counts from register fields (see k_part_count)
        static_assert(kSteps <= 8, "8-bit count fields");
        const FewEdges fe = few_edges(gp, G);
        uint64_t acc = 0;
#pragma unroll
        for (int s = 0; s < kSteps; s++) {
            const int64_t i = base + s * 64 + lane;
            gg[s] = -1;
            if (i < n) {
                kk[s] = keys[i];
                bb[s] = code_at(codes, i, bits);
                gg[s] = few_group(fe, bb[s]);
                acc += 1ull << (8 * gg[s]);
            }
        }
        uint64_t lo, hi;
        few_wave_sum(acc, lo, hi);
        if (lane < G) wb[w][lane] = few_field(lo, hi, lane);
    } else {
#pragma unroll
        for (int s = 0; s < kSteps; s++) {
            const int64_t i = base + s * 64 + lane;
            gg[s] = -1;
            if (i < n) {
                kk[s] = keys[i];
                bb[s] = code_at(codes, i, bits);
                gg[s] = group_of_bin(E, bb[s]);
                atomicAdd(reinterpret_cast<unsigned long long*>(&wb[w][gg[s]]), 1ull);
            }
        }
    }
    __syncthreads();
    // the tile in group order in LDS: wave w's elements of group g at loc[g] + (earlier waves' g)
    if (t < 64) {
        uint32_t c = 0;
        if (lane < G)
            for (int j = 0; j < kWaves; j++) c += (uint32_t)wb[j][lane];
        uint32_t x = c;  // inclusive scan over the groups
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane < G) {
            uint32_t run = x - c;
            gdst[lane] = gbase - (int64_t)run;
            for (int j = 0; j < kWaves; j++) {
                const uint32_t cj = (uint32_t)wb[j][lane];
                wb[j][lane] = run;
                run += cj;
            }
        }
    }
    __syncthreads();
    int nb = 0;
    while ((1 << nb) < G) nb++;
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int s = 0; s < kSteps; s++) {
        const bool valid = gg[s] >= 0;
        uint64_t peers = __ballot(valid);
        for (int b = 0; b < nb; b++) {
            const uint64_t bal = __ballot(valid && ((gg[s] >> b) & 1));
            peers &= ((gg[s] >> b) & 1) ? bal : ~bal;
        }
        if (valid) {
            const int pos = (int)wb[w][gg[s]] + __popcll(peers & lt);
            sk[pos] = kk[s];
            sb[pos] = bb[s];
            sg[pos] = (uint8_t)gg[s];
        }
        // every lane has read its base; the leader of each peer set advances it
        __builtin_amdgcn_wave_barrier();
        if (valid && (peers & lt) == 0) wb[w][gg[s]] += __popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // each group's run of the tile goes out with consecutive lanes on consecutive addresses
    const int tile_n = (int)std::min<int64_t>(kSpTile, n - (int64_t)blockIdx.x * kSpTile);
    for (int q = t; q < tile_n; q += kSpThreads) {
        const int64_t dst = gdst[sg[q]] + q;
        gkeys[dst] = sk[q];
        gbins[dst] = (uint16_t)sb[q];
    }
}

hipError_t launch_part_scatter(hipStream_t st, const int32_t* keys, const void* qpayload, int64_t n,
                               const SpGroups* gp, const uint64_t* tile_base, int32_t* gkeys,
                               uint16_t* gbins) {
    const int64_t tiles = sp_tiles(n, kSpTile);
    if (tiles <= 0) return hipSuccess;
    const int runs = form(SKML_FORM_PART_BALLOT) == 1 ? 0 : 1;  // (0: the ballot-ranked form)
    hipLaunchKernelGGL(k_part_scatter, dim3((unsigned)tiles), dim3(kSpThreads), 0, st, keys,
                       reinterpret_cast<const uint8_t*>(qpayload), n, gp, tile_base, gkeys, gbins, runs);
    return hipGetLastError();
}

// =============================================================================================
// Device-side encode plan: the per-group decisions the reference takes on whole-group
// statistics, made where the statistics are, so an encode never waits on a host round trip.
// =============================================================================================
// MinMaxSketch.compare with Java int wrap (MinMaxSketch.java:80-86)
__device__ __forceinline__ int32_t mm_cmp(int32_t a, int32_t b, int32_t zero) {
    return (int32_t)((uint32_t)mm_dist(a, zero) - (uint32_t)mm_dist(b, zero));
}

// 4-byte MinMax pairs when no group holds bins on both sides of zeroIdx (FSketchUtils.partition:
// group g takes the bins in [edges[g-1], edges[g])).  calGroupEdges puts zeroIdx on an edge
// unless it falls in the last group or two, so this is the common case.
__device__ void mm_plan_narrow(SpGroups* gp, const SpInit& init) {
    int32_t lo = 0, narrow = init.narrow_ok ? 1 : 0;
    for (int g = 0; g < gp->G; g++) {
        const int32_t hi = gp->edges[g];
        if (lo < gp->zero && gp->zero < hi - 1) narrow = 0;  // a bin below zero and one above
        lo = hi > lo ? hi : lo;
    }
    gp->mm_narrow = narrow;
}

// Table from `init` (every field of the reused device struct rewritten), then
// FSketchUtils.calGroupEdges (frequency/FSketchUtils.java:9-28) on the quantizer's zeroIdx and
// binNum, and the MinMaxSketch fill (MinMaxSketch.java:30-33).
__global__ __launch_bounds__(64) void k_sp_plan_edges(const skml_dense_header* __restrict__ h, SpInit init,
                                                      SpGroups* __restrict__ gp) {
    uint32_t* w = reinterpret_cast<uint32_t*>(gp);
    for (int j = threadIdx.x; j < (int)(sizeof(SpGroups) / 4); j += 64) w[j] = 0u;
    __syncthreads();
    for (int j = threadIdx.x; j < kMaxGroups * kMaxRows; j += 64)
        gp->hash_ids[j / kMaxRows][j % kMaxRows] = init.hash_ids[j / kMaxRows][j % kMaxRows];
    if (threadIdx.x) return;
    const int32_t G = init.G;
    gp->G = G;
    gp->rows = init.rows;
    gp->col_ratio = init.col_ratio;
    if (h->status != SKML_OK) {  // "Encounter NaN value": nothing else runs
        gp->status = kSpNan;
        return;
    }
    const int32_t zero = h->zero_idx, bins = h->bin_num;
    gp->zero = zero;
    gp->bin_num = bins;
    gp->fill = mm_cmp(INT32_MIN, INT32_MAX, zero) <= 0 ? INT32_MIN : INT32_MAX;
    if (G == 2) {
        gp->edges[0] = zero;
        gp->edges[1] = bins;
        mm_plan_narrow(gp, init);
        return;
    }
    const int32_t bpg = bins / G;
    int32_t e;
    if (zero < bpg) e = zero;
    else if (bpg == 0) {  // Java: ArithmeticException "/ by zero"
        gp->status = kSpEdges;
        return;
    } else if ((zero % bpg) < (bpg / 2)) e = bpg + zero % bpg;
    else e = zero % bpg;
    for (int32_t i = 0; i < G - 1; i++, e += bpg) gp->edges[i] = e;
    gp->edges[G - 1] = bins;
    mm_plan_narrow(gp, init);
}

// GroupedMinMaxSketch.compOneGroup's shapes (GroupedMinMaxSketch.java:103-121): colNum =
// ceil(size * colRatio) (no multiply-add contraction: the product rounds as in Java).
__global__ __launch_bounds__(64) void k_sp_plan_groups(SpGroups* __restrict__ gp, const uint64_t* __restrict__ sizes,
                                                       int64_t stride) {
    if (gp->status || threadIdx.x) return;
    const int G = gp->G, rows = gp->rows;
    const double ratio = gp->col_ratio;
    int64_t start = 0, cells = 0;
    for (int g = 0; g < G; g++) {
        const int64_t m = (int64_t)sizes[g * stride];
        gp->gstart[g] = start;
        start += m;
        const int32_t cols = m > 0 ? (int32_t)ceil(__dmul_rn((double)m, ratio)) : 1;
        gp->cols[g] = cols;
        gp->inv_cols[g] = __ddiv_rn(1.0, (double)cols);
        gp->tab_off[g] = cells;
        if (m > 0) cells += (int64_t)rows * cols;
        else
            for (int r = 0; r < kMaxRows; r++) gp->hash_ids[g][r] = 0;  // an empty group picks no hashes
    }
    gp->gstart[G] = start;
    gp->ncells = cells;
}

// DeltaAdaptiveEncoder.calOptimalIntervals (binary/DeltaAdaptiveEncoder.java:23-51) in the
// reference's double summation order, every operation rounded on its own.
__device__ void delta_choose(const uint32_t* __restrict__ count, int64_t size, int32_t& bm, int32_t& bk) {
    double prob[32];
    for (int i = 0; i < 32; i++) prob[i] = __ddiv_rn((double)count[i], (double)size);
    double best = 32.0;
    bm = 1;
    bk = 0;
    for (int32_t m = 2, lg = 1; m <= 16; m *= 2, lg++) {
        const int32_t b = 32 / m;
        double sum = 0.0;
        for (int32_t i = 0; i < m; i++) {
            double ip = 0.0;
            for (int32_t j = 0; j < b; j++) ip = __dadd_rn(ip, prob[i * b + j]);
            sum = __dadd_rn(sum, __dmul_rn((double)(i + 1), ip));
        }
        const double t1 = __dadd_rn(__dmul_rn(sum, (double)b), (double)lg);
        if (t1 < best) {
            best = t1;
            bm = m;
            bk = 0;
        }
        const double t2 = __dadd_rn(__dmul_rn(sum, (double)(b + 1)), 1.0);
        if (t2 < best) {
            best = t2;
            bm = m;
            bk = 1;
        }
    }
}

// One lane per group: its interval choice; lane 0 then the order check and kind1_before.
__global__ __launch_bounds__(64) void k_sp_plan_delta(SpGroups* __restrict__ gp, const uint32_t* __restrict__ hist,
                                                      const uint32_t* __restrict__ err) {
    if (gp->status) return;
    const int G = gp->G, g = threadIdx.x;
    if (g < G) {
        const int64_t m = gp->gstart[g + 1] - gp->gstart[g];
        int32_t bm = 1, bk = 0;
        if (m > 0) {
            uint32_t cnt[32];
            for (int i = 0; i < 32; i++) cnt[i] = hist[g * kDeltaHist + i];
            cnt[31] += hist[g * kDeltaHist + 32];  // bitsNeeded 32 cannot occur for positive deltas
            delta_choose(cnt, m, bm, bk);
        }
        gp->m[g] = bm;
        gp->kind[g] = bk;
    }
    __syncthreads();
    if (g) return;
    if (*err) {  // Maths.log2nlz: "Log for <d>" (util/Maths.java:16-21)
        gp->status = kSpOrder;
        return;
    }
    int32_t k1 = 0;
    for (int j = 0; j < G; j++) {
        gp->kind1_before[j] = k1;
        if (gp->kind[j]) k1 += (int32_t)(gp->gstart[j + 1] - gp->gstart[j]);
    }
}

__global__ __launch_bounds__(kSpThreads) void k_sp_zero_edges(const uint64_t* __restrict__ ts, int64_t tiles,
                                                              const SpGroups* __restrict__ gp,
                                                              uint64_t* __restrict__ fw, uint64_t* __restrict__ dw) {
    if (gp->status) return;
    const int64_t i = (int64_t)blockIdx.x * kSpThreads + threadIdx.x;
    if (i > tiles) return;
    const uint64_t f0 = ts[2 * i], d0 = ts[2 * i + 1];
    fw[f0 >> 6] = 0;
    dw[d0 >> 6] = 0;
    if (i < tiles) {
        const uint64_t f1 = ts[2 * i + 2], d1 = ts[2 * i + 3];
        if (f1 > f0) fw[(f1 - 1) >> 6] = 0;
        if (d1 > d0) dw[(d1 - 1) >> 6] = 0;
    } else {  // the trailing word of each stream (n_words = ceil(bits / 64) + 1)
        fw[(f0 >> 6) + 1] = 0;
        dw[(d0 >> 6) + 1] = 0;
    }
}

__global__ __launch_bounds__(64) void k_sp_finalize(SpGroups* __restrict__ gp, const uint64_t* __restrict__ tot) {
    if (gp->status || threadIdx.x) return;
    const int G = gp->G;
    gp->fb[G] = (int64_t)tot[0];
    gp->db[G] = (int64_t)tot[1];
    for (int g = G - 1; g >= 0; g--)  // k_delta_write set the non-empty groups' bases
        if (gp->gstart[g + 1] == gp->gstart[g]) {
            gp->fb[g] = gp->fb[g + 1];
            gp->db[g] = gp->db[g + 1];
        }
}

hipError_t launch_sp_plan_edges(hipStream_t st, const void* qpayload, const SpInit& init, SpGroups* gp) {
    hipLaunchKernelGGL(k_sp_plan_edges, dim3(1), dim3(64), 0, st,
                       reinterpret_cast<const skml_dense_header*>(qpayload), init, gp);
    return hipGetLastError();
}
hipError_t launch_sp_plan_groups(hipStream_t st, SpGroups* gp, const uint64_t* sizes, int64_t stride) {
    hipLaunchKernelGGL(k_sp_plan_groups, dim3(1), dim3(64), 0, st, gp, sizes, stride);
    return hipGetLastError();
}
hipError_t launch_sp_plan_delta(hipStream_t st, SpGroups* gp, const uint32_t* hist, const uint32_t* err) {
    hipLaunchKernelGGL(k_sp_plan_delta, dim3(1), dim3(64), 0, st, gp, hist, err);
    return hipGetLastError();
}
hipError_t launch_sp_finalize(hipStream_t st, SpGroups* gp, const uint64_t* tot) {
    hipLaunchKernelGGL(k_sp_finalize, dim3(1), dim3(64), 0, st, gp, tot);
    return hipGetLastError();
}
hipError_t launch_sp_zero_edges(hipStream_t st, const uint64_t* tile_base, int64_t tiles, const SpGroups* gp,
                                uint64_t* flag_words, uint64_t* delta_words) {
    const unsigned grid = (unsigned)((tiles + 1 + kSpThreads - 1) / kSpThreads);
    hipLaunchKernelGGL(k_sp_zero_edges, dim3(grid), dim3(kSpThreads), 0, st, tile_base, tiles, gp, flag_words,
                       delta_words);
    return hipGetLastError();
}

}  // namespace skml
