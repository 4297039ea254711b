// skml_glm_dense_lowp.hip -- the mini-batch gradient and the validation pass over dense instances whose x
// is stored as fp32, bf16 or fp16 (skml_glm_dense_lowp_data, include/skml.h).  The contract is
// skml_glm_dense.hip's over the exactly widened values: an element is widened to double (through fp32 for
// the 16-bit types, exact for every bit pattern), every product is rounded in double before it is added,
// every sum is one chain of rounded adds from +0.0 in index order.  Only the bytes change, so these
// kernels are built around 16-byte loads of rows that start on 16-byte boundaries (the pitch rule).
//   k_glm_dense_lowp_predict<X, W, LOSS>  a lane owns a batch position and runs its row's chain alone; the
//                                         wave stages 64 rows x 128 bytes through its own LDS slab: one
//                                         16-byte load per lane and 8 rows, widened to fp32 on the way in,
//                                         stored transposed and padded as dwords, read back lane = row and
//                                         widened to double.  The next tile's 8 loads are in flight while
//                                         the chain over the slab runs.  Then loss.loss / -1.0 * loss.grad
//   k_glm_dense_lowp_valid<X, W, LOSS>    the same dot over every row, loss.loss, the confusion counts
//   k_glm_dense_lowp_plus_by<X>           a lane owns the 1 or 2 adjacent columns of a dword; the wave
//                                         streams the window's rows in batch order, kLowpU rows of loads
//                                         in flight ahead of the dependent adds, one chain per column
// The tile arithmetic is skml_glm_dense_lowp.hpp's, shared with tests/glm_dense_lowp_check.cpp; the window
// is skml_glm.hpp's; the losses and the counts are skml_glm_device.hpp's.
#include "skml_device.hpp"
#include "skml_glm_dense_lowp.hpp"
#include "skml_glm_device.hpp"
#include "skml_opt.hpp"

namespace skml {

template <typename X>
constexpr int kLowpE = 16 / (int)sizeof(X);

// The E values of one 16-byte group as fp32: the bits themselves for fp32, a shift (bf16) or
// v_cvt_f32_f16 (fp16) otherwise.
template <typename X>
__device__ __forceinline__ void lowp_widen_group(const u32x4_v& g, float (&v)[kLowpE<X>]) {
    if constexpr (std::is_same<X, float>::value) {
        v[0] = __uint_as_float(g.x);
        v[1] = __uint_as_float(g.y);
        v[2] = __uint_as_float(g.z);
        v[3] = __uint_as_float(g.w);
    } else {
        widen8<X>(g, v);
    }
}

// The lane's kLowpLoads groups of the tile at c0.  at[i]: the 16-byte index of the lane's group of the row of
// load i at c0 = 0, -1 without a row.  A lane without a group (no row, or the group beyond the pitch)
// reads the first 16 bytes of x, which reach no sum, so the loads of a tile issue back to back.
template <int E>
__device__ __forceinline__ void lowp_tile_load(u32x4_v (&v)[kLowpLoads], const u32x4_v* __restrict__ x,
                                               const int64_t (&at)[kLowpLoads], int64_t c0, int64_t pitch, int lane) {
    const bool in = lowp_group_in_pitch<E>(pitch, c0, lane);
#pragma unroll
    for (int i = 0; i < kLowpLoads; i++) v[i] = x[in && at[i] >= 0 ? at[i] + c0 / E : 0];
}

// acc += (double)w[c0 + c] * slab[c][lane] for c = 0 .. N - 1, each product rounded before its add.
template <int E, int N, typename W>
__device__ __forceinline__ void lowp_chain(double& acc, const W* __restrict__ w, int64_t c0, const float* slab, int lane) {
#pragma unroll
    for (int c = 0; c < N; c++) {
        const double p = (double)w[c0 + c] * (double)slab[lowp_slab_index<E>(c, lane)];
        acc += p;
    }
}

// Maths.dot(w, x_row) for the 64 batch positions from jb on, lane = position: +0.0, then
// (double)w[c] * (double)x[row][c] rounded and added for c = 0 .. dim - 1.  slab: the wave's own
// LowpTile<E>::kWaveLds bytes.  A wave's LDS accesses execute in program order and no other wave sees the
// slab, so a wavefront-scope fence (which keeps the compiler to that order) is all that separates a
// tile's stores from its reads and those reads from the next tile's stores.  jb is wave-uniform.
template <typename X, typename W>
__device__ __forceinline__ double lowp_row_dots(const X* __restrict__ x, int64_t dim, int64_t pitch, const GlmWindow& win,
                                                int64_t batch, int64_t jb, const W* __restrict__ w, float* slab) {
    constexpr int E = kLowpE<X>;
    using T = LowpTile<E>;
    const u32x4_v* xg = reinterpret_cast<const u32x4_v*>(x);
    const int lane = threadIdx.x & 63;
    int64_t at[kLowpLoads];
#pragma unroll
    for (int i = 0; i < kLowpLoads; i++) {
        const int64_t j = jb + lowp_load_row(i, lane);
        at[i] = j < batch ? glm_row_of(win, j) * (pitch / E) + lowp_load_group(lane) : -1;
    }
    u32x4_v nxt[kLowpLoads];
    lowp_tile_load<E>(nxt, xg, at, 0, pitch, lane);
    double acc = 0.0;
    for (int64_t c0 = 0; c0 < dim; c0 += T::kC) {
#pragma unroll
        for (int i = 0; i < kLowpLoads; i++) {
            float v[E];
            lowp_widen_group<X>(nxt[i], v);
#pragma unroll
            for (int e = 0; e < E; e++) slab[lowp_slab_index<E>(lowp_load_col<E>(lane, e), lowp_load_row(i, lane))] = v[e];
        }
        if (c0 + T::kC < dim) lowp_tile_load<E>(nxt, xg, at, c0 + T::kC, pitch, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int cn = lowp_tile_cols<E>(dim, c0);
        if (cn == T::kC) {
#pragma unroll 1
            for (int cc = 0; cc < T::kC; cc += kLowpChunk)
                lowp_chain<E, kLowpChunk>(acc, w, c0 + cc, slab + lowp_slab_index<E>(cc, 0), lane);
        } else {
            for (int c = 0; c < cn; c++) lowp_chain<E, 1>(acc, w, c0 + c, slab + lowp_slab_index<E>(c, 0), lane);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    return acc;
}

// blockDim.x = 64 * waves per workgroup; dynamic LDS: LowpTile<E>::kWaveLds bytes per wave.
template <typename X, typename W, int LOSS>
__global__ __launch_bounds__(64 * kLowpMaxWaves) void k_glm_dense_lowp_predict(
    const X* __restrict__ x, const double* __restrict__ label, int64_t dim, int64_t pitch, GlmWindow win, int64_t batch,
    const W* __restrict__ w, double* __restrict__ pre, double* __restrict__ coef, double* __restrict__ loss) {
    extern __shared__ float s_lowp_slabs[];
    const int wave = threadIdx.x >> 6;
    const int64_t jb = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * 64;
    if (jb >= batch) return;  // the whole wave: nothing below crosses waves
    const double acc = lowp_row_dots<X, W>(x, dim, pitch, win, batch, jb, w, s_lowp_slabs + wave * LowpTile<kLowpE<X>>::kSlab);
    const int64_t j = jb + (threadIdx.x & 63);
    if (j < batch) {
        double l, g;
        glm_loss<LOSS>(acc, label[glm_row_of(win, j)], l, g);
        if (pre) pre[j] = acc;
        coef[j] = -1.0 * g;
        if (loss) loss[j] = l;
    }
}

template <typename X, typename W, int LOSS>
__global__ __launch_bounds__(64 * kLowpMaxWaves) void k_glm_dense_lowp_valid(
    const X* __restrict__ x, const double* __restrict__ label, int64_t rows, int64_t dim, int64_t pitch,
    const W* __restrict__ w, double* __restrict__ pre, double* __restrict__ loss, unsigned long long* __restrict__ cnt) {
    extern __shared__ float s_lowp_slabs[];
    __shared__ unsigned long long s_cnt[kValidCounters];
    const int wave = threadIdx.x >> 6;
    const int64_t jb = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * 64;
    const GlmWindow win{0, rows, 0};
    ValidCount vc;
    int cls = kValidNone;
    bool nan = false;
    if (jb < rows) {  // wave-uniform; every wave reaches the counts below
        const double acc = lowp_row_dots<X, W>(x, dim, pitch, win, rows, jb, w, s_lowp_slabs + wave * LowpTile<kLowpE<X>>::kSlab);
        const int64_t row = jb + (threadIdx.x & 63);
        if (row < rows) {
            const double y = label[row];
            double l, g;
            glm_loss<LOSS>(acc, y, l, g);
            if (pre) pre[row] = acc;
            loss[row] = l;
            cls = valid_class(acc, y);
            nan = acc != acc;
        }
    }
    vc.add(cls, nan);
    vc.finish(s_cnt, cnt);
}

// The kV columns of one dword as doubles.
template <typename X>
__device__ __forceinline__ void lowp_widen_word(uint32_t word, double (&v)[LowpCols<kLowpE<X>>::kV]) {
    if constexpr (std::is_same<X, float>::value) {
        v[0] = (double)__uint_as_float(word);
    } else {
        float lo, hi;
        widen2<X>(word, lo, hi);
        v[0] = (double)lo;
        v[1] = (double)hi;
    }
}

// g[k] = +0.0, then (double)x[row_j][k] * coef[j] rounded and added for j = 0 .. batch - 1; count += #{|g[k]| > 1e-8}.
// The row's first element and coef[j] are wave-uniform (scalar loads, one address register per row); the
// wave's load of a row reads 256 contiguous bytes.  A lane whose dword starts past dim loads the row's first
// dword and stores nothing; the chain of a pad column beside a last odd column is never stored or counted.
template <typename X>
__global__ __launch_bounds__(256) void k_glm_dense_lowp_plus_by(const X* __restrict__ x, int64_t dim, int64_t pitch, GlmWindow win,
                                                                int64_t batch, const double* __restrict__ coef,
                                                                double* __restrict__ g, unsigned long long* count) {
    constexpr int E = kLowpE<X>, V = LowpCols<E>::kV;
    __shared__ unsigned long long s_cnt;
    const uint32_t* xw = reinterpret_cast<const uint32_t*>(x);
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * LowpCols<E>::kWaveCols;
    const int64_t k0 = lowp_col_of<E>(base, 0, lane);
    const int64_t word = k0 < dim ? k0 / V : 0;  // the dword of the row the lane loads
    const int64_t row_words = pitch / V;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; v++) acc[v] = 0.0;
    if (base < dim) {  // wave-uniform
        int64_t j = 0;
        for (; j + kLowpU <= batch; j += kLowpU) {
            uint32_t xv[kLowpU];
            // Wave-uniform: unless the window wraps inside these rows they are consecutive, and a row's address is
            // the one before plus the pitch (two scalar adds, where glm_row_of costs a dozen instructions a row,
            // which bound the loop at one wave per SIMD).
            const int64_t first = glm_row_of(win, j);
            if (glm_row_of(win, j + kLowpU - 1) == first + kLowpU - 1) {
                const uint32_t* at = xw + first * row_words + word;
#pragma unroll
                for (int u = 0; u < kLowpU; u++) xv[u] = at[u * row_words];
            } else {
#pragma unroll
                for (int u = 0; u < kLowpU; u++) xv[u] = xw[glm_row_of(win, j + u) * row_words + word];
            }
#pragma unroll
            for (int u = 0; u < kLowpU; u++) {
                const double c = coef[j + u];
                double e[V];
                lowp_widen_word<X>(xv[u], e);
#pragma unroll
                for (int v = 0; v < V; v++) {
                    const double p = e[v] * c;
                    acc[v] += p;
                }
            }
        }
        for (; j < batch; j++) {  // the last batch % kLowpU rows: an exact trip count
            const double c = coef[j];
            double e[V];
            lowp_widen_word<X>(xw[glm_row_of(win, j) * row_words + word], e);
#pragma unroll
            for (int v = 0; v < V; v++) {
                const double p = e[v] * c;
                acc[v] += p;
            }
        }
    }
    LiveCount lc;
#pragma unroll
    for (int v = 0; v < V; v++) {
        const bool on = k0 + v < dim;
        if (on) g[k0 + v] = acc[v];
        lc.add(on && fabs(acc[v]) > 1e-8);  // DenseDoubleGradient.countNNZ
    }
    lc.finish(&s_cnt, count);
}

// ---- launchers ----
template <typename X, typename W>
static hipError_t launch_lowp_predict_xw(hipStream_t st, const skml_glm_dense_lowp_data& d, const GlmWindow& win, int64_t batch,
                                         int loss_kind, const W* w, double* pre, double* coef, double* loss) {
    const int64_t waves = lowp_row_waves(batch);
    const int wpg = lowp_waves_per_group(waves);
    const dim3 grid((unsigned)((waves + wpg - 1) / wpg)), block(64 * wpg);
    const size_t lds = (size_t)wpg * LowpTile<kLowpE<X>>::kWaveLds;
    const X* x = static_cast<const X*>(d.x);
    switch (loss_kind) {
        case SKML_LOSS_L1_LOG:
        case SKML_LOSS_L2_LOG:
            hipLaunchKernelGGL((k_glm_dense_lowp_predict<X, W, kGlmLog>), grid, block, lds, st, x, d.label, d.dim, d.pitch, win, batch, w, pre, coef, loss);
            break;
        case SKML_LOSS_L2_HINGE:
            hipLaunchKernelGGL((k_glm_dense_lowp_predict<X, W, kGlmHinge>), grid, block, lds, st, x, d.label, d.dim, d.pitch, win, batch, w, pre, coef, loss);
            break;
        case SKML_LOSS_L2_SQUARE:
            hipLaunchKernelGGL((k_glm_dense_lowp_predict<X, W, kGlmSquare>), grid, block, lds, st, x, d.label, d.dim, d.pitch, win, batch, w, pre, coef, loss);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <typename X, typename W>
static hipError_t launch_lowp_valid_xw(hipStream_t st, const skml_glm_dense_lowp_data& d, int loss_kind, const W* w, double* pre,
                                       double* loss, unsigned long long* cnt) {
    const int64_t waves = lowp_row_waves(d.rows);
    const int wpg = lowp_waves_per_group(waves);
    const dim3 grid((unsigned)((waves + wpg - 1) / wpg)), block(64 * wpg);
    const size_t lds = (size_t)wpg * LowpTile<kLowpE<X>>::kWaveLds;
    const X* x = static_cast<const X*>(d.x);
    switch (loss_kind) {
        case SKML_LOSS_L1_LOG:
        case SKML_LOSS_L2_LOG:
            hipLaunchKernelGGL((k_glm_dense_lowp_valid<X, W, kGlmLog>), grid, block, lds, st, x, d.label, d.rows, d.dim, d.pitch, w, pre, loss, cnt);
            break;
        case SKML_LOSS_L2_HINGE:
            hipLaunchKernelGGL((k_glm_dense_lowp_valid<X, W, kGlmHinge>), grid, block, lds, st, x, d.label, d.rows, d.dim, d.pitch, w, pre, loss, cnt);
            break;
        case SKML_LOSS_L2_SQUARE:
            hipLaunchKernelGGL((k_glm_dense_lowp_valid<X, W, kGlmSquare>), grid, block, lds, st, x, d.label, d.rows, d.dim, d.pitch, w, pre, loss, cnt);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <typename X>
static hipError_t launch_lowp_plus_by_x(hipStream_t st, const skml_glm_dense_lowp_data& d, const GlmWindow& win, int64_t batch,
                                        const double* coef, double* g, unsigned long long* count) {
    const int64_t waves = lowp_col_waves<kLowpE<X>>(d.dim);
    const int threads = lowp_col_threads(waves);
    const int64_t per = threads / 64;
    hipLaunchKernelGGL(k_glm_dense_lowp_plus_by<X>, dim3((unsigned)((waves + per - 1) / per)), dim3(threads), 0, st,
                       static_cast<const X*>(d.x), d.dim, d.pitch, win, batch, coef, g, count);
    return hipGetLastError();
}

// f(X{}) for the storage type of d.x.
template <typename F>
static hipError_t lowp_by_kind(int x_kind, F f) {
    switch (x_kind) {
        case SKML_X_F32: return f(float{});
        case SKML_X_BF16: return f(bf16_t{});
        case SKML_X_F16: return f(f16_t{});
        default: return hipErrorInvalidValue;
    }
}

static bool lowp_shape_ok(const skml_glm_dense_lowp_data& d) {
    const int64_t e = lowp_elems_per_group(d.x_kind);
    return e > 0 && d.rows >= 1 && d.dim >= 1 && d.pitch >= d.dim && d.pitch % e == 0 && ((uintptr_t)d.x) % 16 == 0;
}

hipError_t launch_glm_dense_lowp_predict(hipStream_t st, const skml_glm_dense_lowp_data& d, int64_t row0, int64_t batch,
                                         int loss_kind, const void* w, int wide, double* pre, double* coef, double* loss) {
    if (!lowp_shape_ok(d) || batch < 1 || batch > d.rows || row0 < 0 || row0 >= d.rows || !coef) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    return lowp_by_kind(d.x_kind, [&](auto xt) {
        using X = decltype(xt);
        return wide ? launch_lowp_predict_xw<X>(st, d, win, batch, loss_kind, static_cast<const double*>(w), pre, coef, loss)
                    : launch_lowp_predict_xw<X>(st, d, win, batch, loss_kind, static_cast<const float*>(w), pre, coef, loss);
    });
}

hipError_t launch_glm_dense_lowp_valid(hipStream_t st, const skml_glm_dense_lowp_data& d, int loss_kind, const void* w, int wide,
                                       double* pre, double* loss, unsigned long long* cnt) {
    if (!lowp_shape_ok(d) || !loss || !cnt) return hipErrorInvalidValue;
    return lowp_by_kind(d.x_kind, [&](auto xt) {
        using X = decltype(xt);
        return wide ? launch_lowp_valid_xw<X>(st, d, loss_kind, static_cast<const double*>(w), pre, loss, cnt)
                    : launch_lowp_valid_xw<X>(st, d, loss_kind, static_cast<const float*>(w), pre, loss, cnt);
    });
}

hipError_t launch_glm_dense_lowp_plus_by(hipStream_t st, const skml_glm_dense_lowp_data& d, int64_t row0, int64_t batch,
                                         const double* coef, double* g, unsigned long long* count) {
    if (!lowp_shape_ok(d) || batch < 1 || batch > d.rows || row0 < 0 || row0 >= d.rows) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    return lowp_by_kind(d.x_kind, [&](auto xt) { return launch_lowp_plus_by_x<decltype(xt)>(st, d, win, batch, coef, g, count); });
}

}  // namespace skml
