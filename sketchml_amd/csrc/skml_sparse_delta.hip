// skml_sparse_delta.hip -- CDNA4 (gfx950) kernels of the sparse codec: the DeltaAdaptive bit stream writer.
//   k_delta_*        DeltaAdaptiveEncoder.encode step 3 (:72-109): per-element bit lengths, a
//                    tile scan, and a writer that packs MSB-first fields (BinaryUtils.setBits) into
//                    an LDS window of 64-bit BitSet words, flushing boundary words atomically.
#include "skml_device.hpp"
#include "skml_sparse.h"
#include "skml_sparse_device.hpp"

namespace skml {

// =============================================================================================
// DeltaAdaptive bit streams
// =============================================================================================
// interval count, flag length, delta length of one element
__device__ __forceinline__ void delta_lens(const DeltaShape& s, int nb, int& iv, int& fl, int& dl) {
    iv = (nb + s.bpi - 1) >> s.shift;
    fl = s.kind ? iv + 1 : s.nf;
    dl = s.bpi * iv;
}

// need[i0, i0 + 8) (one 8-byte load when the run is whole; i0 is a multiple of 8)
__device__ __forceinline__ void load8_need(const uint8_t* __restrict__ need, int64_t i0, int64_t n, uint8_t (&nb)[8]) {
    if (i0 + 8 <= n) {
        const uint2 w = *reinterpret_cast<const uint2*>(need + i0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            nb[j] = (uint8_t)(w.x >> (8 * j));
            nb[4 + j] = (uint8_t)(w.y >> (8 * j));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) nb[j] = i0 + j < n ? need[i0 + j] : (uint8_t)0;
    }
}
// gkeys[i0, i0 + 8) (two 16-byte loads when the run is whole)
__device__ __forceinline__ void load8_keys(const int32_t* __restrict__ k, int64_t i0, int64_t n, int32_t (&key)[8]) {
    if (i0 + 8 <= n) {
        const int4 a = *reinterpret_cast<const int4*>(k + i0), b = *reinterpret_cast<const int4*>(k + i0 + 4);
        key[0] = a.x, key[1] = a.y, key[2] = a.z, key[3] = a.w;
        key[4] = b.x, key[5] = b.y, key[6] = b.z, key[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) key[j] = i0 + j < n ? k[i0 + j] : 0;
    }
}

__global__ __launch_bounds__(kSpThreads) void k_delta_lens(const uint8_t* __restrict__ need, int64_t n,
                                                           const SpGroups* __restrict__ gp,
                                                           uint64_t* __restrict__ tile_sums) {
    if (gp->status) return;
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ uint64_t sh[8];
    load_starts(gp, S);
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * kSpTile + threadIdx.x * 8;
    uint64_t fsum = 0, dsum = 0;
    if (i0 < n) {
        uint8_t nb[8];
        load8_need(need, i0, n, nb);
        int g = group_of_elem(S, i0);
        DeltaShape s = delta_shape(gp, g);
        for (int j = 0; j < 8 && i0 + j < n; j++) {
            const int64_t i = i0 + j;
            while (i >= S[g + 1]) s = delta_shape(gp, ++g);
            int iv, fl, dl;
            delta_lens(s, nb[j], iv, fl, dl);
            fsum += fl;
            dsum += dl;
        }
    }
    uint64_t v[2] = {fsum, dsum}, tot[2];
    block_excl_scan<2>(v, tot, sh);
    if (threadIdx.x == 0) {
        tile_sums[blockIdx.x * 2] = tot[0];
        tile_sums[blockIdx.x * 2 + 1] = tot[1];
    }
}

hipError_t launch_delta_lens(hipStream_t st, const uint8_t* need, int64_t n, const SpGroups* gp,
                             uint64_t* tile_sums) {
    const int64_t tiles = sp_tiles(n, kSpTile);
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_delta_lens, dim3((unsigned)tiles), dim3(kSpThreads), 0, st, need, n, gp, tile_sums);
    return hipGetLastError();
}

constexpr int kFlagWin = (kSpTile * 17 + 63) / 64 + 2;
constexpr int kDeltaWin = (kSpTile * 32 + 63) / 64 + 2;

__global__ __launch_bounds__(kSpThreads) void k_delta_write(const int32_t* __restrict__ gkeys,
                                                            const uint8_t* __restrict__ need, int64_t n,
                                                            SpGroups* __restrict__ gp,
                                                            const uint64_t* __restrict__ tile_base,
                                                            uint64_t* __restrict__ flag_words,
                                                            uint64_t* __restrict__ delta_words) {
    if (gp->status) return;
    __shared__ int64_t S[kMaxGroups + 1];
    __shared__ uint64_t sh[8];
    __shared__ uint64_t fwin[kFlagWin];
    __shared__ uint64_t dwin[kDeltaWin];
    load_starts(gp, S);
    for (int j = threadIdx.x; j < kFlagWin; j += kSpThreads) fwin[j] = 0;
    for (int j = threadIdx.x; j < kDeltaWin; j += kSpThreads) dwin[j] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * kSpTile + threadIdx.x * 8;
    int32_t key[8];
    uint8_t nb[8];
    uint64_t fsum = 0, dsum = 0;
    int g0 = 0;
    // every global read is issued here, before the scan: the tile's bases, the run's keys and
    // lengths, and the key before the run (used when the run does not start its group)
    const uint64_t fbase = tile_base[blockIdx.x * 2], dbase = tile_base[blockIdx.x * 2 + 1];
    int32_t prev0 = 0;
    if (i0 < n) {
        load8_keys(gkeys, i0, n, key);
        load8_need(need, i0, n, nb);
        prev0 = i0 > 0 ? gkeys[i0 - 1] : 0;
        g0 = group_of_elem(S, i0);
        int g = g0;
        DeltaShape s = delta_shape(gp, g);
        for (int j = 0; j < 8; j++) {
            const int64_t i = i0 + j;
            if (i >= n) break;
            while (i >= S[g + 1]) s = delta_shape(gp, ++g);
            int iv, fl, dl;
            delta_lens(s, nb[j], iv, fl, dl);
            fsum += fl;
            dsum += dl;
        }
    }
    uint64_t v[2] = {fsum, dsum}, tot[2];
    block_excl_scan<2>(v, tot, sh);
    const int64_t fw0 = (int64_t)(fbase >> 6) << 6, dw0 = (int64_t)(dbase >> 6) << 6;
    if (i0 < n) {
        int g = g0;
        DeltaShape s = delta_shape(gp, g);
        uint64_t fo = fbase + v[0], dof = dbase + v[1];
        int32_t prev = i0 > S[g] ? prev0 : 0;
        for (int j = 0; j < 8; j++) {
            const int64_t i = i0 + j;
            if (i >= n) break;
            while (i >= S[g + 1]) s = delta_shape(gp, ++g);
            const bool first = i == S[g];
            if (first) {
                gp->fb[g] = (int64_t)fo;
                gp->db[g] = (int64_t)dof;
            }
            const uint32_t d = first ? (uint32_t)key[j] : (uint32_t)key[j] - (uint32_t)prev;
            prev = key[j];
            int iv, fl, dl;
            delta_lens(s, nb[j], iv, fl, dl);
            const uint32_t fv = s.kind ? (uint32_t)((1u << (iv + 1)) - 2u) : (uint32_t)(iv - 1);
            lds_put_bits(fwin, (int64_t)fo - fw0, fv, fl);
            // bitsPerInterval * intervalNeeded <= 32; a 32-bit field holds d itself
            lds_put_bits(dwin, (int64_t)dof - dw0, d, dl);
            fo += fl;
            dof += dl;
        }
    }
    __syncthreads();
    flush_window(fwin, (int64_t)fbase, tot[0], flag_words);
    flush_window(dwin, (int64_t)dbase, tot[1], delta_words);
}

hipError_t launch_delta_write(hipStream_t st, const int32_t* gkeys, const uint8_t* need, int64_t n,
                              SpGroups* gp, const uint64_t* tile_base, uint64_t* flag_words,
                              uint64_t* delta_words) {
    const int64_t tiles = sp_tiles(n, kSpTile);
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_delta_write, dim3((unsigned)tiles), dim3(kSpThreads), 0, st, gkeys, need, n, gp,
                       tile_base, flag_words, delta_words);
    return hipGetLastError();
}

}  // namespace skml
