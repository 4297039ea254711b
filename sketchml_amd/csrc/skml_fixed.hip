// skml_fixed.hip -- CDNA4 (gfx950) kernels of the FixedPointGradient codec
// (ml/gradient/FixedPointGradient.scala:39-75, sketch/binary/BinaryUtils.java:6-29):
//   k_fixed_norm / k_fixed_finish   norm = sqrt(sum v^2) in double as a fixed tree, the header
//   k_fixed_quantize                code = floor(|v| / norm * max) + sigma | sign, packed MSB-first
//                                   into the BitSet word stream
//   k_fixed_decode, k_fixed_decode_sum, k_fixed_codes, k_fixed_times_by
//   k_fixed_decode_sum_step         the decode-sum's walk with the optimiser update of w / m / v in place
//                                   of the fp32 store: the gradient stays the unrounded double
//   k_fixed_decode_sum_live         #{|g| > 1e-8} of the same sums (toAuto's count)
// Every pass streams: 16-byte nontemporal loads of the values, whole 64-bit words of the stream.
// A staging round is 1,024 consecutive elements = exactly 16 b whole words for every width b, so no
// word is shared between waves and nothing is atomic; a wave owns four consecutive rounds (4,096
// elements, 64 b words) of the quantize pass and jumps the sigma stream once for them.
#include <algorithm>

#include "skml_device.hpp"
#include "skml_opt.hpp"

namespace skml {

constexpr int kFxThreads = 256;
constexpr int kFxWaves = kFxThreads / 64;
constexpr int kFxSub = 1024;            // elements per staging round
constexpr int kFxTile = 4 * kFxSub;     // elements per wave tile of the quantize pass
constexpr int kFxSubWordsMax = 16 * kFxMaxBits;  // 464 words of a round at 29 bits
constexpr int kFxLutBits = 8;           // decode: widths up to this look their 2^b values up in LDS
// Minimum waves per SIMD asked of the register allocator (A/B builds: other values).
#ifndef SKML_FX_Q_WAVES
#define SKML_FX_Q_WAVES 4
#endif
#ifndef SKML_FX_D_WAVES
#define SKML_FX_D_WAVES 4
#endif
#ifndef SKML_FX_S_WAVES
#define SKML_FX_S_WAVES 3  // the decode-sum's forms (sum, step, live) for widths 2, 4, 8, 16 (4 spills); the general forms keep 2
#endif

template <typename X>
struct FxVec;
template <>
struct FxVec<float> {
    typedef float T __attribute__((ext_vector_type(4)));
    static constexpr int V = 4;
};
template <>
struct FxVec<double> {
    typedef double T __attribute__((ext_vector_type(2)));
    static constexpr int V = 2;
};

// The 16 values of one lane in the round starting at element sb (a multiple of 1,024): load m takes
// elements sb + (64 m + lane) V .. + V - 1 (V = 4 floats or 2 doubles: one 16-byte load), v[m V + k].
// The partial last round loads element by element, zero past n.
template <typename X>
__device__ __forceinline__ void fx_load_sub(const X* __restrict__ x, int64_t sb, int64_t n, int lane, X (&v)[16]) {
    constexpr int V = FxVec<X>::V, L = 16 / V;
    typedef typename FxVec<X>::T VT;
    if (sb + kFxSub <= n) {
        const VT* src = reinterpret_cast<const VT*>(x + sb);
#pragma unroll
        for (int m = 0; m < L; m++) {
            const VT t = __builtin_nontemporal_load(src + m * 64 + lane);
#pragma unroll
            for (int k = 0; k < V; k++) v[m * V + k] = t[k];
        }
    } else {
#pragma unroll
        for (int m = 0; m < L; m++)
#pragma unroll
            for (int k = 0; k < V; k++) {
                const int64_t e = sb + (m * 64 + lane) * V + k;
                v[m * V + k] = e < n ? x[e] : (X)0;
            }
    }
}

// Sum of a double over the wave, the same value in every lane: a butterfly, so the order of the
// additions is fixed (a + b == b + a bit for bit).
__device__ __forceinline__ double fx_wave_sum(double v) {
    v += lane_xor<1>(v);
    v += lane_xor<2>(v);
    v += lane_xor<4>(v);
    v += lane_xor<8>(v);
    v += lane_xor<16>(v);
    v += lane_xor<32>(v);
    return v;
}

// =============================================================================================
// Norm: values.foreach(v => norm += v * v) (FixedPointGradient.scala:41-43) as a fixed tree.  A
// lane adds its 16 squares of a round in four chains of 4, the round's sum to its running sum (at
// most 2^21 rounds / 4,096 waves = 512), then the butterfly, the workgroup's 4 waves in order, and
// k_fixed_finish the <= 1,024 workgroup partials (4 per thread, butterfly, 4 waves): no chain of
// additions is longer than 600, every term is >= 0, so the relative error is < 601 * 2^-53.
// =============================================================================================
template <typename X>
__global__ __launch_bounds__(kFxThreads) void k_fixed_norm(const X* __restrict__ x, int64_t n,
                                                           FxPartial* __restrict__ part) {
    __shared__ double s_sum[kFxWaves];
    __shared__ uint32_t s_nz[kFxWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * kFxWaves, wid = (int64_t)blockIdx.x * kFxWaves + wave;
    const int64_t subs = (n + kFxSub - 1) / kFxSub;
    double acc = 0.0;
    bool nz = false;
    for (int64_t s = wid; s < subs; s += nwaves) {
        X v[16];
        fx_load_sub(x, s * kFxSub, n, lane, v);
        double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const double d = (double)v[i];
            a[i & 3] += d * d;
            nz |= d != 0.0;  // NaN counts: it reaches the norm anyway
        }
        acc += (a[0] + a[1]) + (a[2] + a[3]);
    }
    acc = fx_wave_sum(acc);
    const bool any = __ballot(nz) != 0;
    if (lane == 0) {
        s_sum[wave] = acc;
        s_nz[wave] = any ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        FxPartial p;
        p.sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        p.flags = s_nz[0] | s_nz[1] | s_nz[2] | s_nz[3];
        p.pad = 0;
        part[blockIdx.x] = p;
    }
}

// One workgroup: the partials' sum, norm = Math.sqrt, the header, zeros in the header's padding and
// in the words' padding to 256 bytes (the payload's bytes are a function of input, width and seed).
__global__ __launch_bounds__(kFxThreads) void k_fixed_finish(const FxPartial* __restrict__ part, int nparts, int64_t n,
                                                             int bits, int64_t seed, uint8_t* __restrict__ payload) {
    __shared__ double s_sum[kFxWaves];
    __shared__ uint32_t s_nz[kFxWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a = 0.0;
    uint32_t fl = 0;
    for (int i = threadIdx.x; i < nparts; i += kFxThreads) {
        a += part[i].sum;
        fl |= part[i].flags;
    }
    a = fx_wave_sum(a);
    const bool any = __ballot(fl != 0) != 0;
    if (lane == 0) {
        s_sum[wave] = a;
        s_nz[wave] = any ? 1u : 0u;
    }
    __syncthreads();
    uint64_t* p64 = reinterpret_cast<uint64_t*>(payload);
    if (threadIdx.x == 0) {
        const double total = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        const double norm = sqrt(total);
        const bool nonzero = (s_nz[0] | s_nz[1] | s_nz[2] | s_nz[3]) != 0;
        const uint64_t nb = (uint64_t)__double_as_longlong(norm);
        const bool finite = (nb & 0x7FF0000000000000ULL) != 0x7FF0000000000000ULL;  // NaN and inf values end here too
        skml_fixed_header h;
        h.magic = SKML_FIXED_MAGIC;
        h.status = (!finite || (norm == 0.0 && nonzero)) ? SKML_E_NAN : SKML_OK;
        h.n = n;
        h.num_bits = bits;
        h.reserved0 = 0;
        h.norm = norm;
        h.words_offset = kFxHeaderBytes;
        h.seed = seed;
        h.reserved[0] = h.reserved[1] = 0;
        *reinterpret_cast<skml_fixed_header*>(payload) = h;
    } else if (threadIdx.x >= sizeof(skml_fixed_header) / 8 && threadIdx.x < kFxHeaderBytes / 8) {
        p64[threadIdx.x] = 0ull;
    }
    const int64_t nwords = fixed_words(n, bits), padded = (nwords + 31) / 32 * 32;
    if (nwords + (int64_t)threadIdx.x < padded) p64[kFxHeaderBytes / 8 + nwords + threadIdx.x] = 0ull;
}

hipError_t launch_fixed_norm(hipStream_t st, const void* x, int wide, int64_t n, int bits, int64_t seed,
                             FxPartial* part, void* payload) {
    const int64_t subs = (n + kFxSub - 1) / kFxSub;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((subs + kFxWaves - 1) / kFxWaves, kFxMaxParts));
    if (wide)
        hipLaunchKernelGGL(k_fixed_norm<double>, dim3(grid), dim3(kFxThreads), 0, st, static_cast<const double*>(x), n, part);
    else
        hipLaunchKernelGGL(k_fixed_norm<float>, dim3(grid), dim3(kFxThreads), 0, st, static_cast<const float*>(x), n, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fixed_finish, dim3(1), dim3(kFxThreads), 0, st, part, grid, n, bits, seed,
                       reinterpret_cast<uint8_t*>(payload));
    return hipGetLastError();
}

// =============================================================================================
// Quantize + pack.  Lane l of a wave takes elements V l .. V l + V - 1 of every 64 V (one 16-byte
// load), so its sigma draws are: one jump of the table to the tile's first draw on the scalar
// side, (A^(V l), C_(V l)) per lane, then per element one step by (A, C) inside a load and by
// (A^(63 V + 1), C_(63 V + 1)) to the next load -- never a table jump per element.  The codes of a
// round go bit-reversed (setBits writes the most significant bit first) into 4 KB of the wave's LDS;
// lane w then gathers the fields of word w, w + 64, ... and stores whole words, coalesced.
// =============================================================================================
// State after one step by (a, c): a s + c mod 2^48 for s < 2^48, as lcg_step_next1 forms bit 47
// (one v_mad_u64_u32 and two 24-bit multiply-adds for bits 32..47 instead of a 64-bit product).
__device__ __forceinline__ uint64_t lcg_step48(uint64_t a, uint64_t c, uint64_t s) {
    const uint32_t alo = (uint32_t)a, ahi = (uint32_t)(a >> 32), slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
    const uint64_t p = (uint64_t)alo * slo + c;
    uint32_t hi = (uint32_t)(p >> 32);
    asm("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(hi) : "v"(alo), "v"(shi));
    asm("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(hi) : "v"(ahi), "v"(slo));
    return ((uint64_t)(hi & 0xFFFFu) << 32) | (uint32_t)p;
}

template <typename X>
__global__ __launch_bounds__(kFxThreads) __attribute__((amdgpu_waves_per_eu(SKML_FX_Q_WAVES))) void k_fixed_quantize(const X* __restrict__ x, int64_t n,
                                                               uint8_t* __restrict__ payload,
                                                               const uint64_t* __restrict__ jump_tab) {
    __shared__ __align__(16) uint32_t stage[kFxWaves][kFxSub];
    const skml_fixed_header* h = reinterpret_cast<const skml_fixed_header*>(payload);
    if (h->status != SKML_OK) return;  // a refused input has no codes
    const int b = h->num_bits;
    const double norm = h->norm;
    const uint32_t sign = 1u << (b - 1), maxv = sign - 1u, field = (sign << 1) - 1u;
    const double dmax = (double)maxv;
    uint64_t* words = reinterpret_cast<uint64_t*>(payload + kFxHeaderBytes);
    const int64_t nwords = fixed_words(n, b);
    const uint64_t s0 = ((uint64_t)h->seed ^ kLcgMult) & kLcgMask;
    constexpr int V = FxVec<X>::V, L = 16 / V;
    constexpr int kOuter = 63 * V + 1;  // draws from a load's last element to the next load's first
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // level 0 of the jump table: entry m is (A^m, C_m), m < 256
    const uint64_t la = jump_tab[2 * V * lane], lc = jump_tab[2 * V * lane + 1];
    const uint64_t ao = jump_tab[2 * kOuter], co = jump_tab[2 * kOuter + 1];
    uint32_t* st = stage[wave];
    const int64_t nwaves = (int64_t)gridDim.x * kFxWaves, wid = (int64_t)blockIdx.x * kFxWaves + wave;
    const int64_t tiles = (n + kFxTile - 1) / kFxTile;
    const int nw = 16 * b;  // words of a round
    for (int64_t tile = wid; tile < tiles; tile += nwaves) {
        const int64_t base = tile * kFxTile;
        // the state whose bit 47 is sigma of element `base`: base + 1 steps (< 2^32: n < 2^31)
        uint64_t s = lcg_jump_uniform(jump_tab, s0, (uint64_t)base + 1);
        s = (la * s + lc) & kLcgMask;
        for (int sub = 0; sub < kFxTile / kFxSub; sub++) {
            const int64_t sb = base + (int64_t)sub * kFxSub;
            if (sb >= n) break;
            X v[16];
            fx_load_sub(x, sb, n, lane, v);
#pragma unroll
            for (int m = 0; m < L; m++) {
                uint32_t r[V];
#pragma unroll
                for (int k = 0; k < V; k++) {
                    const double d = (double)v[m * V + k];
                    const uint32_t sigma = (uint32_t)(s >> 47) & 1u;
                    s = k == V - 1 ? lcg_step48(ao, co, s) : lcg_step48(kLcgMult, kLcgAdd, s);
                    // Math.floor(Math.abs(v) / norm * max).toInt: a NaN quotient (norm 0) gives 0
                    const double q = floor(fabs(d) / norm * dmax);
                    uint32_t c = (q == q ? (uint32_t)(int)fmin(q, 1073741824.0) : 0u) + sigma;
                    if (d < 0.0) c |= sign;  // -0.0 gets no sign
                    if (sb + (m * 64 + lane) * V + k >= n) c = 0u;  // the partial last tile zero-fills
                    r[k] = __brev(c & field) >> (32 - b);
                }
                if constexpr (V == 4)
                    reinterpret_cast<uint4*>(st)[m * 64 + lane] = make_uint4(r[0], r[1], r[2], r[3]);
                else
                    reinterpret_cast<uint2*>(st)[m * 64 + lane] = make_uint2(r[0], r[1]);
            }
            __builtin_amdgcn_wave_barrier();
            const int64_t w0 = (sb >> 6) * b;  // sb is a multiple of 64
            for (int w = lane; w < nw; w += 64) {
                if (w0 + w >= nwords) break;
                const int bit0 = w * 64;
                int i = bit0 / b;
                int sh = i * b - bit0;  // <= 0: the first field may begin in the word before
                uint64_t acc = (uint64_t)st[i] >> (-sh);
                // fields beginning inside the word; i stays < 1,024 (the round ends on a word boundary)
                for (i++, sh += b; sh < 64; i++, sh += b) acc |= (uint64_t)st[i] << sh;
                __builtin_nontemporal_store(acc, words + w0 + w);
            }
            __builtin_amdgcn_wave_barrier();  // the stage is read before the next round overwrites it
        }
    }
}

hipError_t launch_fixed_quantize(hipStream_t st, const void* x, int wide, int64_t n, void* payload,
                                 const uint64_t* jump_tab) {
    const int64_t tiles = (n + kFxTile - 1) / kFxTile;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((tiles + kFxWaves - 1) / kFxWaves, 2048));
    uint8_t* pl = reinterpret_cast<uint8_t*>(payload);
    if (wide)
        hipLaunchKernelGGL(k_fixed_quantize<double>, dim3(grid), dim3(kFxThreads), 0, st, static_cast<const double*>(x), n,
                           pl, jump_tab);
    else
        hipLaunchKernelGGL(k_fixed_quantize<float>, dim3(grid), dim3(kFxThreads), 0, st, static_cast<const float*>(x), n, pl,
                           jump_tab);
    return hipGetLastError();
}

// =============================================================================================
// Decode: the same round in reverse.  The round's 16 b words go coalesced into the wave's LDS (the
// next round's, or the next payload's, are in flight meanwhile), every lane extracts the fields of
// its 16 elements (a field may straddle two words) and stores 16-byte vectors.
// =============================================================================================
// toArray's value of code c (FixedPointGradient.scala:69-71): divide, then multiply.
__device__ __forceinline__ double fx_value(uint32_t c, uint32_t maxv, uint32_t sign, double dmax, double norm) {
    const double v = (double)(int)(c & maxv) / dmax * norm;
    return (c & sign) ? -v : v;
}
// Field i of the round staged in W as the stream holds it: the code's bits in reverse order (stream
// bit j of a field is bit b - 1 - j of the code).  BinaryUtils.getBits of it is fx_unrev; the LDS
// value tables are indexed by the field itself, which saves the reversal per element.
__device__ __forceinline__ uint32_t fx_field(const uint64_t* W, int i, int b, uint32_t fmask) {
    const int bit = i * b, w = bit >> 6, sh = bit & 63;
    uint64_t f = W[w] >> sh;
    if (sh + b > 64) f |= W[w + 1] << (64 - sh);  // inside the round: it ends on a word boundary
    return (uint32_t)f & fmask;
}
__device__ __forceinline__ uint32_t fx_unrev(uint32_t r, int b) { return __brev(r << (32 - b)); }
// Words lane, lane + 64, ... of the round whose first word is w0 (zero past the stream's end).
__device__ __forceinline__ void fx_load_words(const uint64_t* __restrict__ words, int64_t w0, int64_t nwords, int nw,
                                              int lane, uint64_t (&r)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int w = lane + 64 * j;
        r[j] = (w < nw && w0 + w < nwords) ? __builtin_nontemporal_load(words + w0 + w) : 0ull;
    }
}
__device__ __forceinline__ void fx_stage_words(uint64_t* W, int nw, int lane, const uint64_t (&r)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int w = lane + 64 * j;
        if (w < nw) W[w] = r[j];
    }
}
static_assert(kFxSubWordsMax <= 8 * 64, "a lane holds at most 8 words of a round");

template <typename O>
__global__ __launch_bounds__(kFxThreads) __attribute__((amdgpu_waves_per_eu(SKML_FX_D_WAVES))) void k_fixed_decode(const uint8_t* __restrict__ payload, O* __restrict__ out,
                                                             int64_t n) {
    __shared__ uint64_t stage[kFxWaves][kFxSubWordsMax];
    __shared__ double lut[1 << kFxLutBits];
    const skml_fixed_header* h = reinterpret_cast<const skml_fixed_header*>(payload);
    const int b = h->num_bits;
    if (h->magic != SKML_FIXED_MAGIC || b < kFxMinBits || b > kFxMaxBits) return;  // not a payload: nothing is indexed by it
    const double norm = h->norm;
    const uint32_t sign = 1u << (b - 1), maxv = sign - 1u, fmask = (sign << 1) - 1u;
    const double dmax = (double)maxv;
    const bool use_lut = b <= kFxLutBits;
    if (use_lut)
        for (int r = threadIdx.x; r < (1 << b); r += kFxThreads) lut[r] = fx_value(fx_unrev((uint32_t)r, b), maxv, sign, dmax, norm);
    __syncthreads();
    const uint64_t* words = reinterpret_cast<const uint64_t*>(payload + kFxHeaderBytes);
    const int64_t nwords = fixed_words(h->n, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t* W = stage[wave];
    const int64_t nwaves = (int64_t)gridDim.x * kFxWaves, wid = (int64_t)blockIdx.x * kFxWaves + wave;
    const int64_t subs = (n + kFxSub - 1) / kFxSub;
    const int nw = 16 * b;
    constexpr int V = 16 / sizeof(O), L = 16 / V;
    typedef O VT __attribute__((ext_vector_type(V)));
    uint64_t r[8];
    int64_t s = wid;
    if (s < subs) fx_load_words(words, s * nw, nwords, nw, lane, r);
    for (; s < subs; s += nwaves) {
        fx_stage_words(W, nw, lane, r);
        __builtin_amdgcn_wave_barrier();
        if (s + nwaves < subs) fx_load_words(words, (s + nwaves) * nw, nwords, nw, lane, r);
        const int64_t sb = s * kFxSub;
        const bool full = sb + kFxSub <= n;
#pragma unroll
        for (int m = 0; m < L; m++) {
            VT o;
#pragma unroll
            for (int k = 0; k < V; k++) {
                const uint32_t r = fx_field(W, (m * 64 + lane) * V + k, b, fmask);
                o[k] = (O)(use_lut ? lut[r] : fx_value(fx_unrev(r, b), maxv, sign, dmax, norm));
            }
            const int64_t e0 = sb + (m * 64 + lane) * V;
            if (full) {
                __builtin_nontemporal_store(o, reinterpret_cast<VT*>(out + e0));
            } else {
#pragma unroll
                for (int k = 0; k < V; k++)
                    if (e0 + k < n) out[e0 + k] = o[k];
            }
        }
        __builtin_amdgcn_wave_barrier();  // the stage is read before the next round overwrites it
    }
}

static int fx_stream_grid(int64_t n) {
    const int64_t subs = (n + kFxSub - 1) / kFxSub;
    return (int)std::max<int64_t>(1, std::min<int64_t>((subs + kFxWaves - 1) / kFxWaves, 2048));
}

hipError_t launch_fixed_decode(hipStream_t st, const void* payload, void* out, int wide, int64_t n) {
    if (n <= 0) return hipSuccess;
    const uint8_t* pl = reinterpret_cast<const uint8_t*>(payload);
    if (wide)
        hipLaunchKernelGGL(k_fixed_decode<double>, dim3(fx_stream_grid(n)), dim3(kFxThreads), 0, st, pl,
                           static_cast<double*>(out), n);
    else
        hipLaunchKernelGGL(k_fixed_decode<float>, dim3(fx_stream_grid(n)), dim3(kFxThreads), 0, st, pl,
                           static_cast<float*>(out), n);
    return hipGetLastError();
}

// Fused decode of P payloads of one width and n (the host checked the headers) + sum in double from
// +0.0 in payload order + scale (Gradient.sum, ml/gradient/Gradient.scala:44-49).  A wave walks the
// payloads of a round one after another through its stage, 16 double sums per lane in registers, so
// any P takes the same kernel; widths up to 8 bits look the P x 2^b values up in dynamic LDS.
// POW2: b is 2, 4, 8 or 16, so no field straddles a word and a lane's four consecutive fields are
// one aligned 4 b-bit piece of the stage (one LDS read instead of four to eight).  (The lanes
// loading their pieces straight from the stream, without the stage, ran twice as long: 2.11
// against 1.11 ms for 8 payloads of 2^28 8-bit codes.)
// The walk is one function for its three consumers: done(sb, full, lane, acc) gets the round's
// unscaled sums, acc[4 m + k] of element sb + (64 m + lane) 4 + k, and is reached by every lane of
// the wave; `full` says that the round lies inside n.
constexpr int kFxMaxSumPayloads = 16;
template <bool POW2, typename F>
__device__ __forceinline__ void fx_sum_rounds(const uint8_t* __restrict__ payloads, int P, size_t stride, int64_t n, int b,
                                              uint64_t (*stage)[kFxSubWordsMax], double* s_norm, double* slut, F&& done) {
    const uint32_t sign = 1u << (b - 1), maxv = sign - 1u, fmask = (sign << 1) - 1u;
    const double dmax = (double)maxv;
    const bool use_lut = b <= kFxLutBits;
    if ((int)threadIdx.x < P)
        s_norm[threadIdx.x] = reinterpret_cast<const skml_fixed_header*>(payloads + (size_t)threadIdx.x * stride)->norm;
    if (use_lut)
        for (int i = threadIdx.x; i < (P << b); i += kFxThreads) {
            const double norm = reinterpret_cast<const skml_fixed_header*>(payloads + (size_t)(i >> b) * stride)->norm;
            slut[i] = fx_value(fx_unrev((uint32_t)i & fmask, b), maxv, sign, dmax, norm);
        }
    __syncthreads();
    const int64_t nwords = fixed_words(n, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t* W = stage[wave];
    const int64_t nwaves = (int64_t)gridDim.x * kFxWaves, wid = (int64_t)blockIdx.x * kFxWaves + wave;
    const int64_t subs = (n + kFxSub - 1) / kFxSub;
    const int nw = 16 * b;
    auto words_of = [&](int p) {
        return reinterpret_cast<const uint64_t*>(payloads + (size_t)p * stride + kFxHeaderBytes);
    };
    uint64_t r[8];
    int64_t s = wid;
    if (s < subs) fx_load_words(words_of(0), s * nw, nwords, nw, lane, r);
    for (; s < subs; s += nwaves) {
        double acc[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc[e] = 0.0;
        for (int p = 0; p < P; p++) {
            fx_stage_words(W, nw, lane, r);
            __builtin_amdgcn_wave_barrier();
            if (p + 1 < P) fx_load_words(words_of(p + 1), s * nw, nwords, nw, lane, r);
            else if (s + nwaves < subs) fx_load_words(words_of(0), (s + nwaves) * nw, nwords, nw, lane, r);
            const double norm = s_norm[p];
            const double* t = slut + ((size_t)p << b);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                uint64_t piece = 0;
                if constexpr (POW2) {
                    const int c = m * 64 + lane;
                    piece = b == 8 ? reinterpret_cast<const uint32_t*>(W)[c]
                            : b == 4 ? reinterpret_cast<const uint16_t*>(W)[c]
                            : b == 16 ? W[c] : reinterpret_cast<const uint8_t*>(W)[c];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t f = POW2 ? (uint32_t)(piece >> (k * b)) & fmask
                                            : fx_field(W, (m * 64 + lane) * 4 + k, b, fmask);
                    acc[m * 4 + k] += use_lut ? t[f] : fx_value(fx_unrev(f, b), maxv, sign, dmax, norm);
                }
            }
            __builtin_amdgcn_wave_barrier();  // the stage is read before the next payload overwrites it
        }
        const int64_t sb = s * kFxSub;
        done(sb, sb + kFxSub <= n, lane, acc);
    }
}

template <bool POW2>
__global__ __launch_bounds__(kFxThreads) __attribute__((amdgpu_waves_per_eu(POW2 ? SKML_FX_S_WAVES : 2))) void k_fixed_decode_sum(
    const uint8_t* __restrict__ payloads, int P, size_t stride, float* __restrict__ out, int64_t n, double scale, int b) {
    __shared__ uint64_t stage[kFxWaves][kFxSubWordsMax];
    __shared__ double s_norm[kFxMaxSumPayloads];
    extern __shared__ double slut[];  // P << b doubles when b <= kFxLutBits
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    fx_sum_rounds<POW2>(payloads, P, stride, n, b, stage, s_norm, slut,
                        [&](int64_t sb, bool full, int lane, const double (&acc)[16]) {
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const f32x4 o = {(float)(acc[4 * m] * scale), (float)(acc[4 * m + 1] * scale), (float)(acc[4 * m + 2] * scale),
                             (float)(acc[4 * m + 3] * scale)};
            const int64_t e0 = sb + (m * 64 + lane) * 4;
            if (full) {
                __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(out + e0));
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (e0 + k < n) out[e0 + k] = o[k];
            }
        }
    });
}

// The same walk with the optimiser update in place of the fp32 store (skml_opt.hpp): g = acc * scale
// stays the double it is.  A lane owns four consecutive elements per m step -- one 16-byte vector of
// fp32 state, two of fp64 -- and takes the state one m step at a time, so that at most four
// elements' w, m, v are live beside the 16 sums.  Every element has one owner: the update is in
// place.  LIVE: a full vector whose four elements are all dead (|g| <= 1e-8) is not stored; the
// partial last round goes element by element.  The waves asked for are the decode-sum's: the
// aligned-piece forms take 140-143 registers, which is 3 waves whether 2 or 3 are asked for, and
// spill 44-52 bytes per lane at 4.
template <bool POW2, typename W, bool ADAM>
__global__ __launch_bounds__(kFxThreads) __attribute__((amdgpu_waves_per_eu(POW2 ? SKML_FX_S_WAVES : 2))) void k_fixed_decode_sum_step(
    const uint8_t* __restrict__ payloads, int P, size_t stride, int64_t n, double scale, int b, OptConsts k,
    W* __restrict__ pw, W* __restrict__ pm, W* __restrict__ pv) {
    __shared__ uint64_t stage[kFxWaves][kFxSubWordsMax];
    __shared__ double s_norm[kFxMaxSumPayloads];
    extern __shared__ double slut[];
    fx_sum_rounds<POW2>(payloads, P, stride, n, b, stage, s_norm, slut,
                        [&](int64_t sb, bool full, int lane, const double (&acc)[16]) {
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const double g[4] = {acc[4 * m] * scale, acc[4 * m + 1] * scale, acc[4 * m + 2] * scale, acc[4 * m + 3] * scale};
            const int64_t e0 = sb + (m * 64 + lane) * 4;
            if (full) {
                StateN<ADAM, W, 4> st;
                st.load(pw, pm, pv, e0);
                st.apply(g, k);
                if (!k.live || fabs(g[0]) > 1e-8 || fabs(g[1]) > 1e-8 || fabs(g[2]) > 1e-8 || fabs(g[3]) > 1e-8)
                    st.store(pw, pm, pv, e0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (e0 + j < n) opt_apply_at<ADAM>(g[j], pw, pm, pv, e0 + j, k);
            }
        }
    });
}

// #{|g| > 1e-8} of the same sums into *count (toAuto's count, as k_decode_sum_live's for dense
// payloads).  The rounds are the wave's, so every lane reaches every ballot.
template <bool POW2>
__global__ __launch_bounds__(kFxThreads) __attribute__((amdgpu_waves_per_eu(POW2 ? SKML_FX_S_WAVES : 2))) void k_fixed_decode_sum_live(
    const uint8_t* __restrict__ payloads, int P, size_t stride, int64_t n, double scale, int b, unsigned long long* count) {
    __shared__ uint64_t stage[kFxWaves][kFxSubWordsMax];
    __shared__ double s_norm[kFxMaxSumPayloads];
    __shared__ unsigned long long s_cnt;
    extern __shared__ double slut[];
    LiveCount lc;
    fx_sum_rounds<POW2>(payloads, P, stride, n, b, stage, s_norm, slut,
                        [&](int64_t sb, bool full, int lane, const double (&acc)[16]) {
#pragma unroll
        for (int e = 0; e < 16; e++)
            lc.add((full || sb + ((e >> 2) * 64 + lane) * 4 + (e & 3) < n) && fabs(acc[e] * scale) > 1e-8);
    });
    lc.finish(&s_cnt, count);
}

static size_t fx_sum_lds(int P, int bits) { return bits <= kFxLutBits ? sizeof(double) * ((size_t)P << bits) : 0; }
static bool fx_pow2(int bits) { return bits == 2 || bits == 4 || bits == 8 || bits == 16; }
static bool fx_sum_args_ok(int P, int bits) {
    return P >= 1 && P <= kFxMaxSumPayloads && bits >= kFxMinBits && bits <= kFxMaxBits;
}

hipError_t launch_fixed_decode_sum(hipStream_t st, const void* payloads, int P, size_t stride, float* out,
                                   int64_t n, double scale, int bits) {
    if (n <= 0) return hipSuccess;
    if (!fx_sum_args_ok(P, bits)) return hipErrorInvalidValue;
    const size_t lds = fx_sum_lds(P, bits);
    if (fx_pow2(bits))
        hipLaunchKernelGGL(k_fixed_decode_sum<true>, dim3(fx_stream_grid(n)), dim3(kFxThreads), lds, st,
                           reinterpret_cast<const uint8_t*>(payloads), P, stride, out, n, scale, bits);
    else
        hipLaunchKernelGGL(k_fixed_decode_sum<false>, dim3(fx_stream_grid(n)), dim3(kFxThreads), lds, st,
                           reinterpret_cast<const uint8_t*>(payloads), P, stride, out, n, scale, bits);
    return hipGetLastError();
}

template <bool POW2, typename W>
static void launch_fixed_step_w(hipStream_t st, const uint8_t* pl, int P, size_t stride, int64_t n, double scale, int bits,
                                const OptConsts& k, void* w, void* m, void* v) {
    const dim3 grid(fx_stream_grid(n)), block(kFxThreads);
    const size_t lds = fx_sum_lds(P, bits);
    if (k.adam)
        hipLaunchKernelGGL((k_fixed_decode_sum_step<POW2, W, true>), grid, block, lds, st, pl, P, stride, n, scale, bits, k,
                           static_cast<W*>(w), static_cast<W*>(m), static_cast<W*>(v));
    else
        hipLaunchKernelGGL((k_fixed_decode_sum_step<POW2, W, false>), grid, block, lds, st, pl, P, stride, n, scale, bits, k,
                           static_cast<W*>(w), static_cast<W*>(m), static_cast<W*>(v));
}

hipError_t launch_fixed_decode_sum_step(hipStream_t st, const void* payloads, int P, size_t stride, int64_t n,
                                        double scale, int bits, const OptConsts& k, int wide, void* w, void* m, void* v) {
    if (n <= 0) return hipSuccess;
    if (!fx_sum_args_ok(P, bits)) return hipErrorInvalidValue;
    const uint8_t* pl = reinterpret_cast<const uint8_t*>(payloads);
    if (fx_pow2(bits)) {
        if (wide) launch_fixed_step_w<true, double>(st, pl, P, stride, n, scale, bits, k, w, m, v);
        else launch_fixed_step_w<true, float>(st, pl, P, stride, n, scale, bits, k, w, m, v);
    } else {
        if (wide) launch_fixed_step_w<false, double>(st, pl, P, stride, n, scale, bits, k, w, m, v);
        else launch_fixed_step_w<false, float>(st, pl, P, stride, n, scale, bits, k, w, m, v);
    }
    return hipGetLastError();
}

hipError_t launch_fixed_decode_sum_live(hipStream_t st, const void* payloads, int P, size_t stride, int64_t n,
                                        double scale, int bits, unsigned long long* count) {
    if (n <= 0) return hipSuccess;
    if (!fx_sum_args_ok(P, bits)) return hipErrorInvalidValue;
    const uint8_t* pl = reinterpret_cast<const uint8_t*>(payloads);
    if (fx_pow2(bits))
        hipLaunchKernelGGL(k_fixed_decode_sum_live<true>, dim3(fx_stream_grid(n)), dim3(kFxThreads), fx_sum_lds(P, bits), st,
                           pl, P, stride, n, scale, bits, count);
    else
        hipLaunchKernelGGL(k_fixed_decode_sum_live<false>, dim3(fx_stream_grid(n)), dim3(kFxThreads), fx_sum_lds(P, bits), st,
                           pl, P, stride, n, scale, bits, count);
    return hipGetLastError();
}

// The codes as int32, element by element (a test and parity view, not a hot path); 0 past the
// payload's own n.
__global__ void k_fixed_codes(const uint8_t* __restrict__ payload, int32_t* __restrict__ codes, int64_t n) {
    const skml_fixed_header* h = reinterpret_cast<const skml_fixed_header*>(payload);
    const int b = h->num_bits;
    if (h->magic != SKML_FIXED_MAGIC || b < kFxMinBits || b > kFxMaxBits) return;
    const uint64_t* words = reinterpret_cast<const uint64_t*>(payload + kFxHeaderBytes);
    const int64_t have = h->n;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        uint32_t c = 0;
        if (e < have) {
            const int64_t bit = e * b, w = bit >> 6;
            const int sh = (int)(bit & 63);
            uint64_t f = words[w] >> sh;
            if (sh + b > 64) f |= words[w + 1] << (64 - sh);  // the field's end lies inside the stream
            c = __brev((uint32_t)f << (32 - b));
        }
        codes[e] = (int32_t)c;
    }
}

hipError_t launch_fixed_codes(hipStream_t st, const void* payload, int32_t* codes, int64_t n) {
    if (n <= 0) return hipSuccess;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_fixed_codes, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(payload), codes, n);
    return hipGetLastError();
}

__global__ void k_fixed_times_by(uint8_t* payload, double x) {
    reinterpret_cast<skml_fixed_header*>(payload)->norm *= x;
}

hipError_t launch_fixed_times_by(hipStream_t st, void* payload, double x) {
    hipLaunchKernelGGL(k_fixed_times_by, dim3(1), dim3(1), 0, st, reinterpret_cast<uint8_t*>(payload), x);
    return hipGetLastError();
}

}  // namespace skml
