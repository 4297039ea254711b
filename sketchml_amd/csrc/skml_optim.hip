// skml_optim.hip -- the optimiser update on the device (ml/objective/GradientDescent.scala:104-117,
// ml/objective/Adam.scala:50-77), the consumer of Gradient.sum:
//   k_decode_sum_step      the decode-sum's occupancy form (k_decode_sum_occ, skml_dense.hip) with the
//                          update in place of the fp32 store: the gradient stays the unrounded double
//   k_decode_sum_step_gen  the same for > 8 payloads, mixed code widths and tables beyond the LDS bound
//   k_decode_sum_live      #{|g| > 1e-8} of the same sum (toAuto's count)
//   k_opt_step / k_opt_count / k_opt_step_kv   the update from a dense array and from keys + values
// One __device__ function (opt_apply, skml_opt.hpp) holds the arithmetic; every form calls it.
#include <algorithm>

#include "skml_codes.hpp"
#include "skml_device.hpp"
#include "skml_opt.hpp"

namespace skml {

// Waves per SIMD asked of the fused form (a minimum: the register allocator's cap).  SGD on fp32
// state adds 8 registers to the decode-sum's lane and keeps its values.  Adam holds 24 (fp32) or 48
// (fp64) registers of state and 8 elements' double temporaries, so it asks for one step less
// wherever the decode-sum's value made it spill (DESIGN.md "Optimiser update" has the compiled counts).
template <int BITS, typename W, bool ADAM>
constexpr int step_waves() {
#ifdef SKML_STEP_WAVES  // A/B builds: one value for every instantiation
    return SKML_STEP_WAVES;
#endif
    if (sizeof(W) == 8) return BITS >= 8 ? 3 : 4;
    if (ADAM) return BITS >= 16 ? 3 : 4;  // 5 still spills 16 bytes per lane at 1-4 bits
    return BITS >= 8 ? SKML_OCC_WAVES : SKML_OCC_WAVES_NARROW;
}

// Occupancy form: k_decode_sum_occ<BITS, true> (P <= 8 tables of doubles in dynamic LDS, 8 elements
// per lane, the next step's codes prefetched through address-space-1 pointers).  The lane's loads of
// w / m / v are issued before the table lookups, so they are in flight with them; every element is
// owned by exactly one lane, so the update is in place.
template <int BITS, typename W, bool ADAM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(step_waves<BITS, W, ADAM>()))) void k_decode_sum_step(
    const uint8_t* __restrict__ payloads, int P, size_t stride, int64_t n, double scale, int tab, OptConsts k,
    W* __restrict__ pw, W* __restrict__ pm, W* __restrict__ pv) {
    extern __shared__ double lt[];  // P tables of `tab` doubles
    __shared__ const uint8_t* s_codes[kOccMaxP];
    for (int p = 0; p < P; p++) {
        const uint8_t* pl = payloads + (size_t)p * stride;
        const skml_dense_header* h = reinterpret_cast<const skml_dense_header*>(pl);
        const double* sp = reinterpret_cast<const double*>(pl + kHeaderBytes);
        if (threadIdx.x == 0) s_codes[p] = pl + h->codes_offset;
        for (int b = threadIdx.x; b < h->bin_num; b += 256) lt[p * tab + b] = lut_value(h, sp, b);
    }
    __syncthreads();
    constexpr int kW = occ_words<BITS, kOptPer>();  // code words per payload per step
    const int64_t full = n / kOptPer, gstep = (int64_t)gridDim.x * 256;
    int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t wn[kOccMaxP][kW];
#pragma unroll
    for (int q = 0; q < kOccMaxP; q++)
        if (q < P && g < full) load_codes_occ<BITS, kOptPer>(s_codes[q], g * kOptPer, wn[q]);
    for (; g < full; g += gstep) {
        uint32_t cw[kOccMaxP][kW];
#pragma unroll
        for (int q = 0; q < kOccMaxP; q++)
#pragma unroll
            for (int j = 0; j < kW; j++) cw[q][j] = wn[q][j];
        StateN<ADAM, W, kOptPer> s;
        s.load(pw, pm, pv, g * kOptPer);
        if (g + gstep < full) {
#pragma unroll
            for (int q = 0; q < kOccMaxP; q++)
                if (q < P) load_codes_occ<BITS, kOptPer>(s_codes[q], (g + gstep) * kOptPer, wn[q]);
        }
        double acc[kOptPer];
#pragma unroll
        for (int e = 0; e < kOptPer; e++) acc[e] = 0.0;
#pragma unroll
        for (int q = 0; q < kOccMaxP; q++) {
            if (q >= P) break;
            const double* t = lt + q * tab;
#pragma unroll
            for (int e = 0; e < kOptPer; e++) acc[e] += t[code_occ_at<BITS, kOptPer>(cw[q], e)];
        }
#pragma unroll
        for (int e = 0; e < kOptPer; e++) acc[e] = acc[e] * scale;
        s.apply(acc, k);
        s.store(pw, pm, pv, g * kOptPer);
    }
    if (blockIdx.x == 0 && threadIdx.x < kOptPer) {  // the last n % 8 elements
        const int64_t e = full * kOptPer + threadIdx.x;
        if (e < n) {
            double a = 0.0;
            for (int p = 0; p < P; p++) a += lt[p * tab + read_code(s_codes[p], e, BITS)];
            opt_apply_at<ADAM>(a * scale, pw, pm, pv, e, k);
        }
    }
}

// 8 consecutive codes of one payload starting at e0 (a multiple of 8), any width: one load.
__device__ __forceinline__ void load_codes8(const uint8_t* codes, int64_t e0, int bits, uint32_t (&w)[4]) {
    switch (bits) {
        case 16: {
            const uint4 v = *reinterpret_cast<const uint4*>(codes + 2 * e0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            break;
        }
        case 8: {
            const uint2 v = *reinterpret_cast<const uint2*>(codes + e0);
            w[0] = v.x; w[1] = v.y;
            break;
        }
        case 4: w[0] = *reinterpret_cast<const uint32_t*>(codes + e0 / 2); break;
        case 2: w[0] = *reinterpret_cast<const uint16_t*>(codes + e0 / 4); break;
        default: w[0] = codes[e0 / 8]; break;
    }
}
__device__ __forceinline__ uint32_t code8_at(const uint32_t (&w)[4], int e, int bits) {
    switch (bits) {
        case 16: return (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
        case 8: return (w[e >> 2] >> (8 * (e & 3))) & 255u;
        case 4: return (w[0] >> (4 * e)) & 15u;
        case 2: return (w[0] >> (2 * e)) & 3u;
        default: return (w[0] >> e) & 1u;
    }
}

// What the generic forms share: the payloads' code pointers, widths and value tables in LDS
// (k_decode_sum's: tables of at most kSumLutBins bins, wider ones from the payload's splits).
struct GenTables {
    double lut[kMaxSumPayloads][kSumLutBins];
    const uint8_t* codes[kMaxSumPayloads];
    int bits[kMaxSumPayloads], lds[kMaxSumPayloads];
};
__device__ __forceinline__ void gen_fill(GenTables& t, const uint8_t* __restrict__ payloads, int P, size_t stride) {
    for (int p = 0; p < P; p++) {
        const uint8_t* pl = payloads + (size_t)p * stride;
        const skml_dense_header* h = reinterpret_cast<const skml_dense_header*>(pl);
        const double* sp = reinterpret_cast<const double*>(pl + kHeaderBytes);
        const bool in_lds = h->bin_num <= kSumLutBins;
        if (threadIdx.x == 0) {
            t.codes[p] = pl + h->codes_offset;
            t.bits[p] = h->code_bits;
            t.lds[p] = in_lds ? 1 : 0;
        }
        if (in_lds)
            for (int b = threadIdx.x; b < h->bin_num; b += 256) t.lut[p][b] = lut_value(h, sp, b);
    }
    __syncthreads();
}
__device__ __forceinline__ double gen_value(const GenTables& t, const uint8_t* __restrict__ payloads, size_t stride,
                                            int p, uint32_t c) {
    if (t.lds[p]) return t.lut[p][c];
    const uint8_t* pl = payloads + (size_t)p * stride;
    return lut_value(reinterpret_cast<const skml_dense_header*>(pl), reinterpret_cast<const double*>(pl + kHeaderBytes),
                     (int)c);
}
// sum_p v_p[e0 + e], e in [0, 8), from +0.0 in payload order
__device__ __forceinline__ void gen_sum8(const GenTables& t, const uint8_t* __restrict__ payloads, int P, size_t stride,
                                         int64_t e0, double (&acc)[8]) {
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] = 0.0;
    for (int p0 = 0; p0 < P; p0 += kSumChunk) {
        uint32_t cw[kSumChunk][4];
#pragma unroll
        for (int q = 0; q < kSumChunk; q++)
            if (p0 + q < P) load_codes8(t.codes[p0 + q], e0, __builtin_amdgcn_readfirstlane(t.bits[p0 + q]), cw[q]);
#pragma unroll
        for (int q = 0; q < kSumChunk; q++) {
            if (p0 + q >= P) break;
            const int bits = __builtin_amdgcn_readfirstlane(t.bits[p0 + q]);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += gen_value(t, payloads, stride, p0 + q, code8_at(cw[q], e, bits));
        }
    }
}
__device__ __forceinline__ double gen_sum1(const GenTables& t, const uint8_t* __restrict__ payloads, int P, size_t stride,
                                           int64_t e) {
    double a = 0.0;
    for (int p = 0; p < P; p++) a += gen_value(t, payloads, stride, p, read_code(t.codes[p], e, t.bits[p]));
    return a;
}

// Generic fused form (k_decode_sum<0>'s role): any P <= 16, per-payload code widths, any table size.
// The same sum, the same update, the same bits as the occupancy form.
template <typename W, bool ADAM>
__global__ __launch_bounds__(256) void k_decode_sum_step_gen(const uint8_t* __restrict__ payloads, int P, size_t stride,
                                                             int64_t n, double scale, OptConsts k, W* __restrict__ pw,
                                                             W* __restrict__ pm, W* __restrict__ pv) {
    __shared__ GenTables t;
    gen_fill(t, payloads, P, stride);
    const int64_t full = n / kOptPer, gstep = (int64_t)gridDim.x * 256;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < full; g += gstep) {
        StateN<ADAM, W, kOptPer> s;
        s.load(pw, pm, pv, g * kOptPer);
        double acc[kOptPer];
        gen_sum8(t, payloads, P, stride, g * kOptPer, acc);
#pragma unroll
        for (int e = 0; e < kOptPer; e++) acc[e] = acc[e] * scale;
        s.apply(acc, k);
        s.store(pw, pm, pv, g * kOptPer);
    }
    if (blockIdx.x == 0 && threadIdx.x < kOptPer) {
        const int64_t e = full * kOptPer + threadIdx.x;
        if (e < n) opt_apply_at<ADAM>(gen_sum1(t, payloads, P, stride, e) * scale, pw, pm, pv, e, k);
    }
}

__global__ __launch_bounds__(256) void k_decode_sum_live(const uint8_t* __restrict__ payloads, int P, size_t stride,
                                                         int64_t n, double scale, unsigned long long* count) {
    __shared__ GenTables t;
    __shared__ unsigned long long s_cnt;
    gen_fill(t, payloads, P, stride);
    const int64_t full = n / kOptPer, gstep = (int64_t)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    LiveCount lc;
    // the trip count is the wave's, not the lane's: the ballots below need every lane
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); base < full; base += gstep) {
        const bool on = base + lane < full;
        double acc[kOptPer] = {};
        if (on) gen_sum8(t, payloads, P, stride, (base + lane) * kOptPer, acc);
#pragma unroll
        for (int e = 0; e < kOptPer; e++) lc.add(on && fabs(acc[e] * scale) > 1e-8);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int64_t e = full * kOptPer + threadIdx.x;
        const bool on = threadIdx.x < kOptPer && e < n;
        const double a = on ? gen_sum1(t, payloads, P, stride, e) : 0.0;
        lc.add(on && fabs(a * scale) > 1e-8);
    }
    lc.finish(&s_cnt, count);
}

// Array form: the gradient is a dense device array (the output of skml_sparse_decode_sum_f64 or
// skml_fixed_decode_sum_f32, or an uncompressed gradient): g_i = (double)x_i * scale.  One pass.
template <typename G, typename W, bool ADAM>
__global__ __launch_bounds__(256) void k_opt_step(const G* __restrict__ x, int64_t n, double scale, OptConsts k,
                                                  W* __restrict__ pw, W* __restrict__ pm, W* __restrict__ pv) {
    const int64_t full = n / kOptPer, gstep = (int64_t)gridDim.x * 256;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < full; g += gstep) {
        G xv[kOptPer];
        load_state(x, g * kOptPer, xv);
        StateN<ADAM, W, kOptPer> s;
        s.load(pw, pm, pv, g * kOptPer);
        double gr[kOptPer];
#pragma unroll
        for (int e = 0; e < kOptPer; e++) gr[e] = (double)xv[e] * scale;
        s.apply(gr, k);
        s.store(pw, pm, pv, g * kOptPer);
    }
    if (blockIdx.x == 0 && threadIdx.x < kOptPer) {
        const int64_t e = full * kOptPer + threadIdx.x;
        if (e < n) opt_apply_at<ADAM>((double)x[e] * scale, pw, pm, pv, e, k);
    }
}

template <typename G>
__global__ __launch_bounds__(256) void k_opt_count(const G* __restrict__ x, int64_t n, double scale,
                                                   unsigned long long* count) {
    __shared__ unsigned long long s_cnt;
    const int64_t full = n / kOptPer, gstep = (int64_t)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    LiveCount lc;
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); base < full; base += gstep) {
        const bool on = base + lane < full;
        G xv[kOptPer] = {};
        if (on) load_state(x, (base + lane) * kOptPer, xv);
#pragma unroll
        for (int e = 0; e < kOptPer; e++) lc.add(on && fabs((double)xv[e] * scale) > 1e-8);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int64_t e = full * kOptPer + threadIdx.x;
        const bool on = threadIdx.x < kOptPer && e < n;
        lc.add(on && fabs((double)(on ? x[e] : G(0)) * scale) > 1e-8);
    }
    lc.finish(&s_cnt, count);
}

// Key / value form (update(SparseDoubleGradient, ...), Adam.scala:63-77, GradientDescent.scala:111-117):
// w / m / v gathered and scattered at the keys.  The keys are strictly increasing
// (SparseDoubleGradient's invariant), so every element has one owner; a key outside [0, dim) is
// skipped, never written through.
template <typename G, typename W, bool ADAM>
__global__ __launch_bounds__(256) void k_opt_step_kv(const int32_t* __restrict__ keys, const G* __restrict__ vals,
                                                     int64_t nnz, int64_t dim, double scale, OptConsts k,
                                                     W* __restrict__ pw, W* __restrict__ pm, W* __restrict__ pv) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * 256) {
        const int64_t key = keys[i];
        if (key < 0 || key >= dim) continue;
        opt_apply_at<ADAM>((double)vals[i] * scale, pw, pm, pv, key, k);
    }
}

// ---- launchers ----
static unsigned opt_grid(int64_t items, int64_t cap) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, cap));
}

template <int BITS, typename W, bool ADAM>
static void launch_step_occ(hipStream_t st, const uint8_t* pl, int P, size_t stride, int64_t n, double scale,
                            int max_bins, const OptConsts& k, void* w, void* m, void* v) {
    const size_t lds = sizeof(double) * (size_t)max_bins * (size_t)P;
    hipLaunchKernelGGL((k_decode_sum_step<BITS, W, ADAM>), dim3(opt_grid(n / kOptPer, 4096)), dim3(256), lds, st, pl, P,
                       stride, n, scale, max_bins, k, static_cast<W*>(w), static_cast<W*>(m), static_cast<W*>(v));
}
template <typename W, bool ADAM>
static hipError_t launch_step_w(hipStream_t st, const uint8_t* pl, int P, size_t stride, int64_t n, double scale,
                                int common_bits, int max_bins, const OptConsts& k, void* w, void* m, void* v) {
    // the choice between the two forms is launch_decode_sum_o's (skml_dense.hip)
    if ((size_t)max_bins * (size_t)P * sizeof(double) <= kOccLdsMax && P <= kOccMaxP && form(SKML_FORM_DECODE_SUM) != 1) {
        switch (common_bits) {
            case 16: launch_step_occ<16, W, ADAM>(st, pl, P, stride, n, scale, max_bins, k, w, m, v); return hipGetLastError();
            case 8: launch_step_occ<8, W, ADAM>(st, pl, P, stride, n, scale, max_bins, k, w, m, v); return hipGetLastError();
            case 4: launch_step_occ<4, W, ADAM>(st, pl, P, stride, n, scale, max_bins, k, w, m, v); return hipGetLastError();
            case 2: launch_step_occ<2, W, ADAM>(st, pl, P, stride, n, scale, max_bins, k, w, m, v); return hipGetLastError();
            case 1: launch_step_occ<1, W, ADAM>(st, pl, P, stride, n, scale, max_bins, k, w, m, v); return hipGetLastError();
            default: break;  // mixed widths
        }
    }
    hipLaunchKernelGGL((k_decode_sum_step_gen<W, ADAM>), dim3(opt_grid(n / kOptPer, 2048)), dim3(256), 0, st, pl, P, stride,
                       n, scale, k, static_cast<W*>(w), static_cast<W*>(m), static_cast<W*>(v));
    return hipGetLastError();
}

hipError_t launch_decode_sum_step(hipStream_t st, const void* payloads, int P, size_t stride, int64_t n, double scale,
                                  int common_bits, int max_bins, const OptConsts& k, int wide, void* w, void* m,
                                  void* v) {
    if (n <= 0) return hipSuccess;
    if (P < 1 || P > kMaxSumPayloads) return hipErrorInvalidValue;
    const uint8_t* pl = static_cast<const uint8_t*>(payloads);
    if (wide)
        return k.adam ? launch_step_w<double, true>(st, pl, P, stride, n, scale, common_bits, max_bins, k, w, m, v)
                      : launch_step_w<double, false>(st, pl, P, stride, n, scale, common_bits, max_bins, k, w, m, v);
    return k.adam ? launch_step_w<float, true>(st, pl, P, stride, n, scale, common_bits, max_bins, k, w, m, v)
                  : launch_step_w<float, false>(st, pl, P, stride, n, scale, common_bits, max_bins, k, w, m, v);
}

hipError_t launch_decode_sum_live(hipStream_t st, const void* payloads, int P, size_t stride, int64_t n, double scale,
                                  unsigned long long* count) {
    if (n <= 0) return hipSuccess;
    if (P < 1 || P > kMaxSumPayloads) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_decode_sum_live, dim3(opt_grid(n / kOptPer, 2048)), dim3(256), 0, st,
                       static_cast<const uint8_t*>(payloads), P, stride, n, scale, count);
    return hipGetLastError();
}

template <typename G, typename W>
static void launch_opt_step_gw(hipStream_t st, const void* g, int64_t n, double scale, const OptConsts& k, void* w,
                               void* m, void* v) {
    const unsigned grid = opt_grid(n / kOptPer, 8192);
    if (k.adam)
        hipLaunchKernelGGL((k_opt_step<G, W, true>), dim3(grid), dim3(256), 0, st, static_cast<const G*>(g), n, scale, k,
                           static_cast<W*>(w), static_cast<W*>(m), static_cast<W*>(v));
    else
        hipLaunchKernelGGL((k_opt_step<G, W, false>), dim3(grid), dim3(256), 0, st, static_cast<const G*>(g), n, scale, k,
                           static_cast<W*>(w), static_cast<W*>(m), static_cast<W*>(v));
}

hipError_t launch_opt_step(hipStream_t st, const void* g, int g_wide, int64_t n, double scale, const OptConsts& k,
                           int wide, void* w, void* m, void* v) {
    if (n <= 0) return hipSuccess;
    if (g_wide) {
        if (wide) launch_opt_step_gw<double, double>(st, g, n, scale, k, w, m, v);
        else launch_opt_step_gw<double, float>(st, g, n, scale, k, w, m, v);
    } else {
        if (wide) launch_opt_step_gw<float, double>(st, g, n, scale, k, w, m, v);
        else launch_opt_step_gw<float, float>(st, g, n, scale, k, w, m, v);
    }
    return hipGetLastError();
}

hipError_t launch_opt_count(hipStream_t st, const void* g, int g_wide, int64_t n, double scale,
                            unsigned long long* count) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = opt_grid(n / kOptPer, 4096);
    if (g_wide)
        hipLaunchKernelGGL(k_opt_count<double>, dim3(grid), dim3(256), 0, st, static_cast<const double*>(g), n, scale, count);
    else
        hipLaunchKernelGGL(k_opt_count<float>, dim3(grid), dim3(256), 0, st, static_cast<const float*>(g), n, scale, count);
    return hipGetLastError();
}

template <typename G, typename W>
static void launch_opt_kv_gw(hipStream_t st, const int32_t* keys, const void* vals, int64_t nnz, int64_t dim, double scale,
                             const OptConsts& k, void* w, void* m, void* v) {
    const unsigned grid = opt_grid(nnz, 4096);
    if (k.adam)
        hipLaunchKernelGGL((k_opt_step_kv<G, W, true>), dim3(grid), dim3(256), 0, st, keys, static_cast<const G*>(vals), nnz,
                           dim, scale, k, static_cast<W*>(w), static_cast<W*>(m), static_cast<W*>(v));
    else
        hipLaunchKernelGGL((k_opt_step_kv<G, W, false>), dim3(grid), dim3(256), 0, st, keys, static_cast<const G*>(vals), nnz,
                           dim, scale, k, static_cast<W*>(w), static_cast<W*>(m), static_cast<W*>(v));
}

hipError_t launch_opt_step_kv(hipStream_t st, const int32_t* keys, const void* vals, int v_wide, int64_t nnz,
                              int64_t dim, double scale, const OptConsts& k, int wide, void* w, void* m, void* v) {
    if (nnz <= 0) return hipSuccess;
    if (v_wide) {
        if (wide) launch_opt_kv_gw<double, double>(st, keys, vals, nnz, dim, scale, k, w, m, v);
        else launch_opt_kv_gw<double, float>(st, keys, vals, nnz, dim, scale, k, w, m, v);
    } else {
        if (wide) launch_opt_kv_gw<float, double>(st, keys, vals, nnz, dim, scale, k, w, m, v);
        else launch_opt_kv_gw<float, float>(st, keys, vals, nnz, dim, scale, k, w, m, v);
    }
    return hipGetLastError();
}

}  // namespace skml
