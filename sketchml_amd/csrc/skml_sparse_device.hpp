// skml_sparse_device.hpp -- device helpers that more than one file of the sparse codec uses
// (skml_sparse*.hip); private to those files.  Everything here is __forceinline__, a template,
// inline or constexpr; no kernel is defined here.
#pragma once
#include <algorithm>

#include "skml_device.hpp"
#include "skml_sparse.h"

namespace skml {

// look-back status words: the flag in the top two bits, the count below
constexpr uint64_t kStAgg = 1ULL << 62, kStPre = 2ULL << 62, kStMask = (1ULL << 62) - 1;

// ---------------------------------------------------------------------------------------------
// block scan helpers (256 threads)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_incl_u64(uint64_t v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl_up(v, off, 64);
        if (lane >= off) v += y;
    }
    return v;
}

// v[k] -> exclusive prefix over the block; total[k] = block sum.  sh: 4*K u64 of LDS.
template <int K>
__device__ __forceinline__ void block_excl_scan(uint64_t (&v)[K], uint64_t (&total)[K], uint64_t* sh) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint64_t inc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        inc[k] = wave_incl_u64(v[k], lane);
        if (lane == 63) sh[w * K + k] = inc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        uint64_t base = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < kSpThreads / 64; j++) {
            const uint64_t s = sh[j * K + k];
            base += j < w ? s : 0;
            tot += s;
        }
        v[k] = base + inc[k] - v[k];
        total[k] = tot;
    }
    __syncthreads();
}

// Look-back status words carry their payload (flag | count) in the word itself, so relaxed
// agent-scope atomics suffice: no release / acquire fences (an agent release writes back the
// whole L2 -- per tile, that was 30x slower).
__device__ __forceinline__ uint64_t ld_status(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_status(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// group g with gstart[g] <= i < gstart[g+1] (S: G+1 offsets in LDS, padded to 65 with INT64_MAX)
__device__ __forceinline__ int group_of_elem(const int64_t* S, int64_t i) {
    int g = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1)
        if (S[g + step] <= i) g += step;
    return g;
}

__device__ __forceinline__ void load_starts(const SpGroups* gp, int64_t* S) {
    for (int j = threadIdx.x; j <= kMaxGroups; j += blockDim.x) S[j] = j <= gp->G ? gp->gstart[j] : INT64_MAX;
}

// |v - zero| with Java int wrap (MinMaxSketch.compare, MinMaxSketch.java:80-86)
__device__ __forceinline__ int32_t mm_dist(int32_t v, int32_t zero) {
    const int32_t d = (int32_t)((uint32_t)v - (uint32_t)zero);
    return d < 0 ? (int32_t)(0u - (uint32_t)d) : d;
}

// a group's DeltaAdaptive field shape (writer and decoder)
struct DeltaShape {
    int bpi, shift, nf, kind;
};
__device__ __forceinline__ DeltaShape delta_shape(const SpGroups* gp, int g) {
    DeltaShape s;
    const int m = gp->m[g];
    s.bpi = 32 / m;
    s.shift = 31 - __clz(s.bpi);
    s.nf = 31 - __clz(m);
    s.kind = gp->kind[g];
    return s;
}

// BinaryUtils.setBits (binary/BinaryUtils.java:6-14): value's MSB at the lowest bit position.
__device__ __forceinline__ void lds_put_bits(uint64_t* win, int64_t rel, uint32_t value, int nbits) {
    if (nbits <= 0) return;
    const uint64_t rev = (uint64_t)(__brev(value) >> (32 - nbits));
    const int64_t w = rel >> 6;
    const int sh = (int)(rel & 63);
    atomicOr(reinterpret_cast<unsigned long long*>(&win[w]), (unsigned long long)(rev << sh));
    if (sh + nbits > 64) atomicOr(reinterpret_cast<unsigned long long*>(&win[w + 1]), (unsigned long long)(rev >> (64 - sh)));
}

__device__ __forceinline__ void flush_window(const uint64_t* win, int64_t bit0, uint64_t nbits, uint64_t* out) {
    if (nbits == 0) return;
    const int64_t w0 = bit0 >> 6, w1 = (bit0 + (int64_t)nbits - 1) >> 6;
    for (int64_t w = w0 + threadIdx.x; w <= w1; w += kSpThreads) {
        const uint64_t v = win[w - w0];
        if (w == w0 || w == w1) {
            if (v) atomicOr(reinterpret_cast<unsigned long long*>(&out[w]), (unsigned long long)v);
        } else {
            out[w] = v;
        }
    }
}

// workgroups of `kern` (`threads` each) resident at once on the device; 0 if the query fails
template <typename K>
static int resident_blocks(K kern, int threads) {
    int dev = 0, per_cu = 0;
    hipDeviceProp_t prop;
    int r = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, 0) == hipSuccess)
        r = std::max(1, per_cu) * prop.multiProcessorCount;
    (void)hipGetLastError();
    return r;
}

}  // namespace skml
