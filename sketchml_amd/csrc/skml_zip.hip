// skml_zip.hip -- CDNA4 (gfx950) kernels of the ZipMLQuantizer split search
// (ml/gradient/ZipGradient.scala:70-129, sketch/util/Sort.java:43-58):
//   k_zip_keys / k_zip_hist / k_zip_scatter / k_zip_unkey   the sorted copy: an LSD radix sort (8-bit
//                                   digits) of the order-preserving keys, widened to double
//   k_zip_scan_dd                   r = prefix sums of the sorted values, t = of their squares, as a
//                                   fixed tree in compensated arithmetic (no atomics, no look-back:
//                                   the same bits on every run)
//   k_zip_err, k_zip_sel_hist / k_zip_sel_pick, k_zip_cnt / k_zip_compact
//                                   one halving round over splitIndex in global memory: the pairs'
//                                   errors, the thrNum-th largest by a radix select on the 64-bit
//                                   key, the stream compaction of the kept splits
//   k_zip_finish                    every round once splitNum fits one workgroup's LDS, then the
//                                   split table, min and max
// The quantize pass is the dense codec's own (k_set_splits, launch_quantize / launch_quantize64).
// Integer atomics only (histograms, the NaN flag): their results do not depend on the order.
#include <algorithm>

#include "skml_device.hpp"
#include "skml_zip.hpp"

namespace skml {

constexpr int kZuItems = 8;
constexpr int kZuBlock = kZsThreads * kZuItems;  // 2,048 entries per workgroup of the integer scan and of a round
constexpr int kZfThreads = 1024;                 // k_zip_finish
constexpr int kZfWaves = kZfThreads / 64;
static_assert(kZipTail == 4 * kZfThreads, "k_zip_finish: two pairs per thread");

template <typename X>
struct ZipKey;
template <>
struct ZipKey<float> {
    using K = uint32_t;
    static constexpr int kPasses = 4;
    __device__ static __forceinline__ K key(float f) { return zip_key32(f); }
    __device__ static __forceinline__ bool bad(float f) { return zip_bad32(f); }
};
template <>
struct ZipKey<double> {
    using K = uint64_t;
    static constexpr int kPasses = 8;
    __device__ static __forceinline__ K key(double d) { return zip_key64(d); }
    __device__ static __forceinline__ bool bad(double d) { return zip_bad64(d); }
};
__device__ __forceinline__ double zip_value_of(uint32_t k) { return (double)zip_unkey32(k); }  // widening is exact
__device__ __forceinline__ double zip_value_of(uint64_t k) { return zip_unkey64(k); }

static int zip_stream_grid(int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + kZsThreads - 1) / kZsThreads, 4096));
}

// =============================================================================================
// Sort
// =============================================================================================
template <typename X>
__global__ __launch_bounds__(kZsThreads) void k_zip_keys(const X* __restrict__ x, int64_t n,
                                                         typename ZipKey<X>::K* __restrict__ keys, ZipState* st) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kZsThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kZsThreads) {
        const X v = x[i];
        bad |= ZipKey<X>::bad(v);
        keys[i] = ZipKey<X>::key(v);
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(&st->bad, 1);
}

// Digit counts of workgroup b's tile, digit-major: hist[d * nblocks + b].
template <typename K>
__global__ __launch_bounds__(kZsThreads) void k_zip_hist(const K* __restrict__ keys, int64_t n, int pass,
                                                         uint32_t* __restrict__ hist, int nblocks) {
    __shared__ uint32_t h[kZipDigits];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t b0 = (int64_t)blockIdx.x * kZsTile, e = b0 + kZsTile < n ? b0 + kZsTile : n;
    for (int64_t i = b0 + threadIdx.x; i < e; i += kZsThreads) atomicAdd(&h[zip_digit((uint64_t)keys[i], pass)], 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of workgroup b's tile (the tile k_zip_hist counted) to offs[d * nblocks + b] on,
// 1,024 keys at a time in input order: four rows of 256, a thread one key of each.  A key's rank
// among its wave's equal digits of its row comes from eight ballots; the 16 (row, wave) counts of a
// digit are turned into offsets by that digit's thread, which also moves the digit's base on.  Two
// workgroup barriers per 1,024 keys.  Every position is below n because the offsets are the
// exclusive scan of the counts of these same tiles.
static_assert(kZsTile % (kZsRows * kZsThreads) == 0, "a tile is whole steps");
template <typename K>
__global__ __launch_bounds__(kZsThreads) void k_zip_scatter(const K* __restrict__ in, K* __restrict__ out, int64_t n,
                                                            int pass, const uint32_t* __restrict__ offs, int nblocks) {
    constexpr int kSlots = kZsRows * kZsWaves;
    __shared__ uint32_t s_base[kZipDigits];
    __shared__ uint32_t s_cnt[kSlots][kZipDigits];
    __shared__ uint32_t s_off[kSlots][kZipDigits];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_base[tid] = offs[(size_t)tid * nblocks + blockIdx.x];
    for (int q = 0; q < kSlots; q++) s_cnt[q][tid] = 0u;
    __syncthreads();
    const int64_t b0 = (int64_t)blockIdx.x * kZsTile, e = b0 + kZsTile < n ? b0 + kZsTile : n;
    for (int64_t s0 = b0; s0 < e; s0 += kZsRows * kZsThreads) {
        K key[kZsRows];
        int d[kZsRows], rank[kZsRows];
        bool valid[kZsRows];
#pragma unroll
        for (int j = 0; j < kZsRows; j++) {
            const int64_t i = s0 + j * kZsThreads + tid;
            valid[j] = i < e;
            key[j] = valid[j] ? in[i] : (K)0;
        }
#pragma unroll
        for (int j = 0; j < kZsRows; j++) {
            d[j] = valid[j] ? zip_digit((uint64_t)key[j], pass) : 0;
            uint64_t peers = __ballot(valid[j]);
#pragma unroll
            for (int b = 0; b < kZipDigitBits; b++) {
                const bool bit = (d[j] >> b) & 1;
                const uint64_t m = __ballot(valid[j] && bit);
                peers &= bit ? m : ~m;
            }
            rank[j] = __popcll(peers & ((1ull << lane) - 1ull));
            if (valid[j] && rank[j] == 0) s_cnt[j * kZsWaves + wave][d[j]] = (uint32_t)__popcll(peers);
        }
        __syncthreads();
        {  // digit tid: counts -> offsets in (row, wave) order, the counts cleared for the next step
            uint32_t run = s_base[tid];
#pragma unroll
            for (int q = 0; q < kSlots; q++) {
                const uint32_t c = s_cnt[q][tid];
                s_off[q][tid] = run;
                s_cnt[q][tid] = 0u;
                run += c;
            }
            s_base[tid] = run;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kZsRows; j++)
            if (valid[j]) {
                const uint32_t pos = s_off[j * kZsWaves + wave][d[j]] + (uint32_t)rank[j];
                if ((int64_t)pos < n) out[pos] = key[j];
            }
        // the next step writes s_cnt (cleared above) before its first barrier and s_off only after it
    }
}

template <typename K>
__global__ __launch_bounds__(kZsThreads) void k_zip_unkey(const K* __restrict__ keys, int64_t n,
                                                          double* __restrict__ sorted) {
    for (int64_t i = (int64_t)blockIdx.x * kZsThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kZsThreads)
        sorted[i] = zip_value_of(keys[i]);
}

// Exclusive scan of uint32 in place, 2,048 entries per workgroup; totals[b] = the workgroup's sum.
__device__ __forceinline__ uint32_t zip_block_excl_u32(uint32_t sum, uint32_t* s_w, int nwaves, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan_u32(sum);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t off = inc - sum, tot = 0u;
    for (int w = 0; w < nwaves; w++) {
        if (w < wave) off += s_w[w];
        tot += s_w[w];
    }
    *total = tot;
    return off;
}

__global__ __launch_bounds__(kZsThreads) void k_zip_scan_u32(uint32_t* data, int64_t n, uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_w[kZsWaves];
    const int64_t base = (int64_t)blockIdx.x * kZuBlock + (int64_t)threadIdx.x * kZuItems;
    uint32_t v[kZuItems], sum = 0u;
#pragma unroll
    for (int k = 0; k < kZuItems; k++) {
        v[k] = base + k < n ? data[base + k] : 0u;
        sum += v[k];
    }
    uint32_t tot;
    uint32_t run = zip_block_excl_u32(sum, s_w, kZsWaves, &tot);
#pragma unroll
    for (int k = 0; k < kZuItems; k++) {
        if (base + k < n) data[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kZsThreads) void k_zip_add_u32(uint32_t* __restrict__ data, int64_t n,
                                                            const uint32_t* __restrict__ offs) {
    const uint32_t off = offs[blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * kZuBlock;
    for (int k = threadIdx.x; k < kZuBlock; k += kZsThreads)
        if (base + k < n) data[base + k] += off;
}

static int64_t zu_blocks(int64_t n) { return (n + kZuBlock - 1) / kZuBlock; }

// tmp: zip_scan_u32_tmp(n) entries
hipError_t zip_scan_u32(hipStream_t st, uint32_t* data, int64_t n, uint32_t* tmp) {
    const int64_t nb = zu_blocks(n);
    hipLaunchKernelGGL(k_zip_scan_u32, dim3((unsigned)nb), dim3(kZsThreads), 0, st, data, n, tmp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nb <= 1) return e;
    if ((e = zip_scan_u32(st, tmp, nb, tmp + nb)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_zip_add_u32, dim3((unsigned)nb), dim3(kZsThreads), 0, st, data, n, tmp);
    return hipGetLastError();
}
size_t zip_scan_u32_tmp(int64_t n) {
    size_t total = 0;
    for (int64_t nb = zu_blocks(std::max<int64_t>(n, 1));; nb = zu_blocks(nb)) {
        total += (size_t)nb;
        if (nb <= 1) break;
    }
    return total;
}

hipError_t launch_zip_hist64(hipStream_t st, const uint64_t* keys, int64_t n, int pass, uint32_t* hist, int nblocks) {
    hipLaunchKernelGGL(k_zip_hist<uint64_t>, dim3(nblocks), dim3(kZsThreads), 0, st, keys, n, pass, hist, nblocks);
    return hipGetLastError();
}

template <typename X>
static hipError_t zip_sort_t(hipStream_t st, const X* x, int64_t n, const ZipScratch& s, double* sorted) {
    using K = typename ZipKey<X>::K;
    K* a = static_cast<K*>(s.keys_a);
    K* b = static_cast<K*>(s.keys_b);
    const int nblocks = (int)((n + kZsTile - 1) / kZsTile);
    hipLaunchKernelGGL(k_zip_keys<X>, dim3(zip_stream_grid(n)), dim3(kZsThreads), 0, st, x, n, a, s.state);
    hipError_t e = hipGetLastError();
    for (int pass = 0; pass < ZipKey<X>::kPasses && e == hipSuccess; pass++) {
        hipLaunchKernelGGL(k_zip_hist<K>, dim3(nblocks), dim3(kZsThreads), 0, st, a, n, pass, s.hist, nblocks);
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = zip_scan_u32(st, s.hist, (int64_t)kZipDigits * nblocks, s.hist_tmp)) != hipSuccess) break;
        hipLaunchKernelGGL(k_zip_scatter<K>, dim3(nblocks), dim3(kZsThreads), 0, st, a, b, n, pass, s.hist, nblocks);
        e = hipGetLastError();
        std::swap(a, b);  // an even number of passes: the sorted keys end in keys_a
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_zip_unkey<K>, dim3(zip_stream_grid(n)), dim3(kZsThreads), 0, st, a, n, sorted);
    return hipGetLastError();
}

hipError_t launch_zip_sort(hipStream_t st, const void* x, int wide, int64_t n, const ZipScratch& s, double* sorted) {
    return wide ? zip_sort_t<double>(st, static_cast<const double*>(x), n, s, sorted)
                : zip_sort_t<float>(st, static_cast<const float*>(x), n, s, sorted);
}

// =============================================================================================
// Prefix sums r (values) and t (squares), ZipGradient.scala:76-83, as a fixed tree in compensated
// (double-double) arithmetic, rounded to double once at the end.
//
// The tree: a thread adds its 8 consecutive values in order; the 64 thread totals of a wave by a
// Hillis-Steele scan (6 steps); the 4 wave totals in order; output = ((workgroup offset + (wave
// offset + lane offset)) + the thread's own prefix.  The workgroup totals ((w0 + w1) + w2) + w3 go
// through the same tree (k_zip_scan_dd<false> over the totals), reduce first, then scan, so every
// output is rounded exactly once.  zip_scan_depth (skml_zip.hpp) counts the additions behind an
// output; in plain double that alone bounds the error by depth * 2^-53 * sum |s_j|.
//
// Why compensated: a gradient's sorted copy holds long runs of one value, mostly exact zeros.  The
// reference's sequential r does not move along a run of zeros, so a range inside the run has error
// exactly 0, and the search's ties at 0 (which decide whether it terminates at all) depend on it.
// A plain tree associates the values before the run differently for every element of the run, and
// r wobbles in its last bit.  With each partial sum carried as an unevaluated hi + lo pair (error
// about 2^-104 per addition) and the squares taken exactly (s * s = p + fma(s, s, -p)), r and t are
// the correctly rounded exact sums except when the exact sum lies within about depth * 2^-104 of a
// rounding boundary -- constant along runs of zeros, like the reference's.
// =============================================================================================
static_assert(kZipScanThreads == kZsThreads && kZipScanItems == 8, "the scan tree of zip_scan_depth");

struct zdd {
    double hi, lo;
};
// x + y: TwoSum of the high parts, the low parts added in, renormalised (hi = fl(hi + lo)).
__device__ __forceinline__ zdd zdd_add(zdd x, zdd y) {
    const double s = x.hi + y.hi;
    const double bb = s - x.hi;
    double e = (x.hi - (s - bb)) + (y.hi - bb);
    e = e + (x.lo + y.lo);
    const double hi = s + e;
    return {hi, e - (hi - s)};
}
__device__ __forceinline__ zdd zdd_shfl_up(zdd v, int d) { return {__shfl_up(v.hi, d, 64), __shfl_up(v.lo, d, 64)}; }

// LEAF: in_ah = the sorted values (a = s, b = s * s exactly), outputs r -> out_ah, t -> out_bh as
// doubles.  Otherwise the four arrays are (hi, lo) of two sequences of pairs, scanned in place.
// SCAN = false: only the workgroup totals (tot*) are written; SCAN = true: the outputs, each plus
// the inclusive total of the workgroups before it (off*, null for a single workgroup).
struct ZddArrays {
    double *ah, *al, *bh, *bl;
};
template <bool LEAF, bool SCAN>
__global__ __launch_bounds__(kZsThreads) void k_zip_scan_dd(const double* in_s, ZddArrays io, double* out_r, double* out_t,
                                                            ZddArrays tot, ZddArrays off, int64_t n) {
    __shared__ zdd s_wa[kZsWaves], s_wb[kZsWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kZipScanBlock + (int64_t)threadIdx.x * kZipScanItems;
    const zdd zero = {0.0, 0.0};
    zdd a[kZipScanItems], b[kZipScanItems];
#pragma unroll
    for (int k = 0; k < kZipScanItems; k++) {
        a[k] = b[k] = zero;
        if (base + k < n) {
            if constexpr (LEAF) {
                const double v = in_s[base + k], p = v * v;
                a[k] = {v, 0.0};
                b[k] = {p, fma(v, v, -p)};
            } else {
                a[k] = {io.ah[base + k], io.al[base + k]};
                b[k] = {io.bh[base + k], io.bl[base + k]};
            }
        }
    }
#pragma unroll
    for (int k = 1; k < kZipScanItems; k++) {
        a[k] = zdd_add(a[k - 1], a[k]);
        b[k] = zdd_add(b[k - 1], b[k]);
    }
    zdd ta = a[kZipScanItems - 1], tb = b[kZipScanItems - 1];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const zdd ua = zdd_shfl_up(ta, d), ub = zdd_shfl_up(tb, d);
        if (lane >= d) {
            ta = zdd_add(ua, ta);
            tb = zdd_add(ub, tb);
        }
    }
    zdd ea = zdd_shfl_up(ta, 1), eb = zdd_shfl_up(tb, 1);  // the lanes before this one
    if (lane == 0) ea = eb = zero;
    if (lane == 63) {
        s_wa[wave] = ta;
        s_wb[wave] = tb;
    }
    __syncthreads();
    zdd wa = zero, wb = zero;  // the waves before this one, in order
    for (int w = 0; w < wave; w++) {
        wa = zdd_add(wa, s_wa[w]);
        wb = zdd_add(wb, s_wb[w]);
    }
    if constexpr (!SCAN) {
        if (threadIdx.x == kZsThreads - 1) {
            const zdd fa = zdd_add(wa, ta), fb = zdd_add(wb, tb);
            tot.ah[blockIdx.x] = fa.hi;
            tot.al[blockIdx.x] = fa.lo;
            tot.bh[blockIdx.x] = fb.hi;
            tot.bl[blockIdx.x] = fb.lo;
        }
    } else {
        zdd oa = zdd_add(wa, ea), ob = zdd_add(wb, eb);
        if (blockIdx.x > 0) {
            const int64_t p = (int64_t)blockIdx.x - 1;
            oa = zdd_add({off.ah[p], off.al[p]}, oa);
            ob = zdd_add({off.bh[p], off.bl[p]}, ob);
        }
#pragma unroll
        for (int k = 0; k < kZipScanItems; k++)
            if (base + k < n) {
                const zdd ra = zdd_add(oa, a[k]), rb = zdd_add(ob, b[k]);
                if constexpr (LEAF) {
                    out_r[base + k] = ra.hi;
                    out_t[base + k] = rb.hi;
                } else {
                    io.ah[base + k] = ra.hi;
                    io.al[base + k] = ra.lo;
                    io.bh[base + k] = rb.hi;
                    io.bl[base + k] = rb.lo;
                }
            }
    }
}

static int64_t zf_blocks(int64_t n) { return (n + kZipScanBlock - 1) / kZipScanBlock; }
static size_t zip_scan_f64_tmp(int64_t n) {  // pairs per sequence, all tree levels above the leaves
    size_t total = 0;
    for (int64_t nb = zf_blocks(std::max<int64_t>(n, 1));; nb = zf_blocks(nb)) {
        total += (size_t)nb;
        if (nb <= 1) break;
    }
    return total;
}

static ZddArrays zdd_at(const ZddArrays& t, int64_t i) { return {t.ah + i, t.al + i, t.bh + i, t.bl + i}; }

// Inclusive scan of n entries: the leaves (sorted -> r, t) or the pairs `io` in place; `tot`: room
// for the totals of this level and of every level above it.
static hipError_t zip_scan_level(hipStream_t st, bool leaf, const double* sorted, ZddArrays io, double* r, double* t,
                                 int64_t n, ZddArrays tot) {
    const int64_t nb = zf_blocks(n);
    const ZddArrays none = {nullptr, nullptr, nullptr, nullptr};
    const dim3 grid((unsigned)nb), block(kZsThreads);
    if (nb > 1) {
        if (leaf) hipLaunchKernelGGL((k_zip_scan_dd<true, false>), grid, block, 0, st, sorted, io, r, t, tot, none, n);
        else hipLaunchKernelGGL((k_zip_scan_dd<false, false>), grid, block, 0, st, sorted, io, r, t, tot, none, n);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if ((e = zip_scan_level(st, false, nullptr, tot, nullptr, nullptr, nb, zdd_at(tot, nb))) != hipSuccess) return e;
    }
    if (leaf) hipLaunchKernelGGL((k_zip_scan_dd<true, true>), grid, block, 0, st, sorted, io, r, t, none, tot, n);
    else hipLaunchKernelGGL((k_zip_scan_dd<false, true>), grid, block, 0, st, sorted, io, r, t, none, tot, n);
    return hipGetLastError();
}

hipError_t launch_zip_scan(hipStream_t st, const double* sorted, int64_t n, double* r, double* t, const ZipScratch& s) {
    const size_t nt = zip_scan_f64_tmp(n);
    const ZddArrays tot = {s.tot_a, s.tot_a + nt, s.tot_b, s.tot_b + nt};
    const ZddArrays none = {nullptr, nullptr, nullptr, nullptr};
    return zip_scan_level(st, true, sorted, none, r, t, n, tot);
}

// =============================================================================================
// One round over splitIndex in global memory (idx == nullptr: round 1's identity).
// =============================================================================================
__global__ __launch_bounds__(kZsThreads) void k_zip_err(const int32_t* __restrict__ idx, int64_t split_num, int64_t n,
                                                        const double* __restrict__ r, const double* __restrict__ t,
                                                        double* __restrict__ err) {
    const int64_t h = split_num / 2;
    for (int64_t i = (int64_t)blockIdx.x * kZsThreads + threadIdx.x; i < h; i += (int64_t)gridDim.x * kZsThreads) {
        int64_t L, R;
        zip_pair_range(idx, i, split_num, n, &L, &R);
        err[i] = zip_pair_error(r, t, L, R);
    }
}

// Whether a key is still a candidate of the select: equal to `prefix` above digit `pass`.
__device__ __forceinline__ bool zip_sel_match(uint64_t key, uint64_t prefix, int pass) {
    return pass == 7 || (key >> (kZipDigitBits * (pass + 1))) == (prefix >> (kZipDigitBits * (pass + 1)));
}

__global__ __launch_bounds__(kZsThreads) void k_zip_sel_hist(const double* __restrict__ err, int64_t h, int pass,
                                                             ZipState* st) {
    __shared__ uint32_t s_h[kZipDigits];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t prefix = st->prefix;
    for (int64_t i = (int64_t)blockIdx.x * kZsThreads + threadIdx.x; i < h; i += (int64_t)gridDim.x * kZsThreads) {
        const uint64_t key = zip_key64(err[i]);
        if (zip_sel_match(key, prefix, pass)) atomicAdd(&s_h[zip_digit(key, pass)], 1u);
    }
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], s_h[threadIdx.x]);
}

// The digit of this pass: the zeros behind the errors (the rest of the reference's zero-initialised
// array) join the counts, then the walk from the largest digit down.
__global__ void k_zip_sel_pick(ZipState* st, int pass, int64_t nzeros) {
    if (threadIdx.x != 0) return;
    const uint64_t zkey = zip_key64(0.0);
    uint64_t prefix = st->prefix;
    if (nzeros > 0 && zip_sel_match(zkey, prefix, pass)) st->hist[zip_digit(zkey, pass)] += (uint32_t)nzeros;
    int64_t k = st->k;
    const int d = zip_select_digit(st->hist, &k);
    prefix |= (uint64_t)d << (kZipDigitBits * pass);
    st->prefix = prefix;
    st->k = k;
    for (int i = 0; i < kZipDigits; i++) st->hist[i] = 0u;
    if (pass == 0) st->thr = zip_unkey64(prefix);
}

__global__ void k_zip_sel_begin(ZipState* st, int64_t k) {
    if (threadIdx.x != 0) return;
    st->prefix = 0ull;
    st->k = k;
    st->kept = 0;
    for (int i = 0; i < kZipDigits; i++) st->hist[i] = 0u;
}

// Kept pairs of workgroup b's 2,048 pairs.
__global__ __launch_bounds__(kZsThreads) void k_zip_cnt(const double* __restrict__ err, int64_t h, const ZipState* st,
                                                        uint32_t* __restrict__ blockcnt) {
    __shared__ uint32_t s_w[kZsWaves];
    const double thr = st->thr;
    const int64_t base = (int64_t)blockIdx.x * kZuBlock + (int64_t)threadIdx.x * kZuItems;
    uint32_t sum = 0u;
#pragma unroll
    for (int k = 0; k < kZuItems; k++) sum += (base + k < h && err[base + k] >= thr) ? 1u : 0u;
    uint32_t tot;
    (void)zip_block_excl_u32(sum, s_w, kZsWaves, &tot);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = tot;
}

// blockoff: the exclusive scan of k_zip_cnt's counts.  Pair i writes splitIndex[2i] at i + (kept
// pairs before it) and, when kept, splitIndex[2i+1] behind it; an odd split_num's last singleton
// is dropped.  The last pair publishes the kept total.  Positions stay below 2h <= split_num.
__global__ __launch_bounds__(kZsThreads) void k_zip_compact(const int32_t* __restrict__ idx, int32_t* __restrict__ out,
                                                            const double* __restrict__ err, int64_t h, ZipState* st,
                                                            const uint32_t* __restrict__ blockoff) {
    __shared__ uint32_t s_w[kZsWaves];
    const double thr = st->thr;
    const int64_t base = (int64_t)blockIdx.x * kZuBlock + (int64_t)threadIdx.x * kZuItems;
    bool keep[kZuItems];
    uint32_t sum = 0u;
#pragma unroll
    for (int k = 0; k < kZuItems; k++) {
        keep[k] = base + k < h && err[base + k] >= thr;
        sum += keep[k] ? 1u : 0u;
    }
    uint32_t tot;
    int64_t before = (int64_t)blockoff[blockIdx.x] + zip_block_excl_u32(sum, s_w, kZsWaves, &tot);
#pragma unroll
    for (int k = 0; k < kZuItems; k++) {
        const int64_t i = base + k;
        if (i >= h) break;
        const int64_t pos = zip_out_pos(i, before);
        out[pos] = (int32_t)zip_split_at(idx, 2 * i);
        if (keep[k]) {
            out[pos + 1] = (int32_t)zip_split_at(idx, 2 * i + 1);
            before++;
        }
        if (i == h - 1) st->kept = before;
    }
}

hipError_t launch_zip_round(hipStream_t st, const int32_t* idx, int32_t* idx_out, int64_t split_num, int64_t n,
                            int bins, const double* r, const double* t, const ZipScratch& s) {
    const int64_t h = split_num / 2;
    const int grid = zip_stream_grid(h);
    hipLaunchKernelGGL(k_zip_sel_begin, dim3(1), dim3(64), 0, st, s.state, zip_thr_num(split_num, bins));
    hipLaunchKernelGGL(k_zip_err, dim3(grid), dim3(kZsThreads), 0, st, idx, split_num, n, r, t, s.err);
    hipError_t e = hipGetLastError();
    for (int pass = 7; pass >= 0 && e == hipSuccess; pass--) {
        hipLaunchKernelGGL(k_zip_sel_hist, dim3(grid), dim3(kZsThreads), 0, st, s.err, h, pass, s.state);
        hipLaunchKernelGGL(k_zip_sel_pick, dim3(1), dim3(64), 0, st, s.state, pass, split_num - h);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    const int64_t nb = zu_blocks(h);
    hipLaunchKernelGGL(k_zip_cnt, dim3((unsigned)nb), dim3(kZsThreads), 0, st, s.err, h, s.state, s.blockcnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = zip_scan_u32(st, s.blockcnt, nb, s.blockcnt_tmp)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_zip_compact, dim3((unsigned)nb), dim3(kZsThreads), 0, st, idx, idx_out, s.err, h, s.state,
                       s.blockcnt);
    return hipGetLastError();
}

// =============================================================================================
// The tail in one workgroup: while splitNum > bins (and splitNum <= kZipTail on entry), the same
// round with splitIndex, the errors and the select's histogram in LDS; then splits[i] =
// sorted[splitIndex[i + 1]], min, max and binNum.  With split_num > kZipTail on entry the search
// is over (the host ran every round) and only the split table is gathered.
// =============================================================================================
__global__ __launch_bounds__(kZfThreads) void k_zip_finish(const int32_t* __restrict__ idx, int64_t split_num0,
                                                           int64_t n, int bins, const double* __restrict__ r,
                                                           const double* __restrict__ t,
                                                           const double* __restrict__ sorted,
                                                           double* __restrict__ splits, ZipState* st) {
    __shared__ int32_t s_idx[2][kZipTail];
    __shared__ double s_err[kZipTail / 2];
    __shared__ uint32_t s_hist[kZipDigits];
    __shared__ uint32_t s_w[kZfWaves];
    const int tid = threadIdx.x;
    int status = kZipOk, rounds = 0;
    int64_t sn = split_num0;
    if (sn > kZipTail) {
        for (int64_t i = tid; i < sn - 1; i += kZfThreads) splits[i] = sorted[zip_split_at(idx, i + 1)];
    } else {
        int cur = 0;
        for (int i = tid; i < (int)sn; i += kZfThreads) s_idx[0][i] = (int32_t)zip_split_at(idx, i);
        __syncthreads();
        while (sn > bins) {  // sn is the same in every thread
            const int32_t* si = s_idx[cur];
            int32_t* so = s_idx[cur ^ 1];
            const int h = (int)(sn / 2);
            int64_t k = zip_thr_num(sn, bins);
            if (k <= 0) {
                status = kZipThrZero;
                break;
            }
            for (int i = tid; i < h; i += kZfThreads) {
                int64_t L, R;
                zip_pair_range(si, i, sn, n, &L, &R);
                s_err[i] = zip_pair_error(r, t, L, R);
            }
            uint64_t prefix = 0ull;
            const uint64_t zkey = zip_key64(0.0);
            for (int pass = 7; pass >= 0; pass--) {
                if (tid < kZipDigits) s_hist[tid] = 0u;
                __syncthreads();  // also: the errors are written
                for (int i = tid; i < h; i += kZfThreads) {
                    const uint64_t key = zip_key64(s_err[i]);
                    if (zip_sel_match(key, prefix, pass)) atomicAdd(&s_hist[zip_digit(key, pass)], 1u);
                }
                if (tid == 0 && sn - h > 0 && zip_sel_match(zkey, prefix, pass))
                    atomicAdd(&s_hist[zip_digit(zkey, pass)], (uint32_t)(sn - h));
                __syncthreads();
                const int d = zip_select_digit(s_hist, &k);  // every thread walks the same counts
                prefix |= (uint64_t)d << (kZipDigitBits * pass);
                __syncthreads();
            }
            const double thr = zip_unkey64(prefix);
            // pairs 2 tid and 2 tid + 1
            const int i0 = 2 * tid, i1 = 2 * tid + 1;
            const bool k0 = i0 < h && s_err[i0] >= thr, k1 = i1 < h && s_err[i1] >= thr;
            uint32_t tot;
            const uint32_t before = zip_block_excl_u32((k0 ? 1u : 0u) + (k1 ? 1u : 0u), s_w, kZfWaves, &tot);
            if (i0 < h) {
                const int p = (int)zip_out_pos(i0, before);
                so[p] = si[2 * i0];
                if (k0) so[p + 1] = si[2 * i0 + 1];
            }
            if (i1 < h) {
                const int p = (int)zip_out_pos(i1, before + (k0 ? 1u : 0u));
                so[p] = si[2 * i1];
                if (k1) so[p + 1] = si[2 * i1 + 1];
            }
            __syncthreads();
            const int64_t next = (int64_t)h + tot;  // an odd sn's last singleton is dropped
            if (next >= sn) {
                status = kZipNoProgress;
                break;
            }
            sn = next;
            cur ^= 1;
            rounds++;
        }
        if (status == kZipOk)
            for (int i = tid; i < (int)sn - 1; i += kZfThreads) splits[i] = sorted[s_idx[cur][i + 1]];
    }
    if (tid == 0) {
        st->status = status;
        st->bin_num = (int32_t)sn;
        st->rounds = rounds;
        st->mn = sorted[0];
        st->mx = sorted[n - 1];
    }
}

hipError_t launch_zip_finish(hipStream_t st, const int32_t* idx, int64_t split_num, int64_t n, int bins,
                             const double* r, const double* t, const double* sorted, const ZipScratch& s) {
    hipLaunchKernelGGL(k_zip_finish, dim3(1), dim3(kZfThreads), 0, st, idx, split_num, n, bins, r, t, sorted, s.splits,
                       s.state);
    return hipGetLastError();
}

// Scratch of one call over n values (fp32: wide = 0); own_prefix: sorted, r and t are part of it.
size_t zip_scratch_layout(int64_t n, int wide, int own_prefix, ZipScratch* out, char* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return base ? (void*)(base + o) : nullptr;
    };
    const size_t ksz = wide ? 8 : 4, nn = (size_t)n;
    const int64_t nblocks = (n + kZsTile - 1) / kZsTile;
    const int64_t h = n / 2 + 1;
    ZipScratch s;
    s.state = (ZipState*)take(sizeof(ZipState));
    s.keys_a = take(ksz * nn);
    s.keys_b = take(ksz * nn);
    s.idx_a = (int32_t*)s.keys_a;  // the keys are dead once the sorted copy is written
    s.idx_b = (int32_t*)s.keys_b;
    s.sorted = own_prefix ? (double*)take(8 * nn) : nullptr;
    s.r = own_prefix ? (double*)take(8 * nn) : nullptr;
    s.t = own_prefix ? (double*)take(8 * nn) : nullptr;
    s.err = (double*)take(8 * (size_t)h);
    s.hist = (uint32_t*)take(4 * (size_t)kZipDigits * (size_t)nblocks);
    s.hist_tmp = (uint32_t*)take(4 * zip_scan_u32_tmp((int64_t)kZipDigits * nblocks));
    s.blockcnt = (uint32_t*)take(4 * (size_t)zu_blocks(h));
    s.blockcnt_tmp = (uint32_t*)take(4 * zip_scan_u32_tmp(zu_blocks(h)));
    const size_t nt = zip_scan_f64_tmp(n);
    s.tot_a = (double*)take(16 * nt);  // (hi, lo) halves
    s.tot_b = (double*)take(16 * nt);
    s.splits = (double*)take(8 * (size_t)SKML_MAX_BINS);
    if (out) *out = s;
    return off;
}

}  // namespace skml
