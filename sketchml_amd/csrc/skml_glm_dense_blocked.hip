// skml_glm_dense_blocked.hip -- the mini-batch gradient over dense instances in the blocked summation order:
// the opt-in twin of skml_glm_dense.hip and skml_glm_dense_lowp.hip for callers who need a deterministic
// gradient at memory speed and not the bits of Java's sequential `+=`.  One source for the four storages of x
// (double, fp32, bf16, fp16) and both weight types.
//
// The contract.  All arithmetic is in double; a narrow x is widened exactly, as in the sequential kernels.
// Products are fused into their add (v_fma_f64, written as __builtin_fma: the build has -ffp-contract=off).
// pre_j is a sum over all dim columns, g[k] a sum over the batch window rows, and every partial sum starts from
// +0.0.  The order of every sum is a function of batch, dim, the storage type and the constants of
// skml_glm_dense_blocked.hpp (row0 enters only through the window): never of the device, of the grid that
// happened to be resident, of atomics or of timing, so the same call gives the same bits on every run.  No
// floating-point atomic anywhere; the only atomics are LiveCount's integer ones.  coef_j, loss_j (glm_loss on
// this pre_j), objLoss, toAuto's count over the finished g, the outputs and NULL rules are the sequential
// entries'.  NaN and Inf take part as in any IEEE sum; a pad element of a pitched row is loaded and masked to
// +0.0 x +0.0 before it could reach a chain (a chain from +0.0 is never -0.0, so that term changes no bit).
//
//   k_glm_dense_blocked_predict<X, W, LOSS>  L lanes share a row (blk_lanes: the smallest of 8, 16, 32, 64 whose
//       16-byte loads cover it).  A row of at most 64 groups: a lane holds its group of w in registers and
//       loads its group of kBlkRowUnroll rows back to back, 64 / L rows per load instruction, kBlkShortSteps
//       times.  A longer row: a wave (or S waves of one workgroup, when batch alone gives too few waves:
//       blk_split) walks it kBlkRowUnroll segments of 64 groups at a time, x and w by the same 16-byte vector
//       loads wherever the segment's groups are whole, one FMA chain per lane and slot.  The slots are added
//       as (0 + 1) + (2 + 3), the L lanes by a __shfl_xor butterfly from L / 2 down to 1, the S waves through
//       LDS in wave order from +0.0.  The group's first lane applies glm_loss and stores pre, coef and loss.
//       A row of doubles with an odd dim starts on an 8-byte boundary only: such an x (and any x or w off a
//       16-byte boundary) is read by 8-byte loads, element by element, in the same order; nothing is peeled.
//   k_glm_dense_blocked_partial<X>           grid = column strips x NB row blocks.  A lane owns the columns of
//       one 8-byte load and runs their FMA chains over the block's RB window rows, kBlkU rows of loads in
//       flight, coef_j wave-uniform, a row's address the one before plus the pitch unless the step holds the
//       window's wrap.  Block b stores partial[b][dim]; with NB = 1 it stores g itself and counts.
//   k_glm_dense_blocked_reduce               a lane per column adds the NB partials in block order from +0.0,
//       stores g[k] and feeds LiveCount.
// Both legs are matrix-vector products (N = 1) bound by HBM: v_mfma_f64_16x16x4_f64 would compute 16 columns to
// use one, so no matrix instruction appears here.
#include "skml_device.hpp"
#include "skml_glm_dense_blocked.hpp"
#include "skml_glm_device.hpp"
#include "skml_opt.hpp"

namespace skml {

template <typename X>
constexpr int kBlkE = 16 / (int)sizeof(X);

// The E values of one 16-byte group as doubles, exactly.
template <typename X>
__device__ __forceinline__ void blk_widen_group(const u32x4_v& g, double (&v)[kBlkE<X>]) {
    if constexpr (std::is_same<X, double>::value) {
        v[0] = __hiloint2double((int)g.y, (int)g.x);
        v[1] = __hiloint2double((int)g.w, (int)g.z);
    } else if constexpr (std::is_same<X, float>::value) {
        v[0] = (double)__uint_as_float(g.x);
        v[1] = (double)__uint_as_float(g.y);
        v[2] = (double)__uint_as_float(g.z);
        v[3] = (double)__uint_as_float(g.w);
    } else {
        float f[8];
        widen8<X>(g, f);
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = (double)f[e];
    }
}

// The group of E elements at element `at` of x (a multiple of E when x16), whose first column is c.  A lane
// without a group (`valid` false) reads the first bytes of x, which reach no sum, so that the loads of a step
// issue back to back.  x16: rows start on 16-byte boundaries (always for a narrow x: the pitch rule); otherwise
// x holds doubles and each is loaded alone, the second only where the row has it.
template <typename X>
__device__ __forceinline__ u32x4_v blk_load_group(const X* __restrict__ x, int64_t at, int64_t c, int64_t dim, bool x16, bool valid) {
    if constexpr (std::is_same<X, double>::value) {
        if (!x16) {
            const uint2* xq = reinterpret_cast<const uint2*>(x);
            const uint2 a = xq[valid ? at : 0], b = xq[valid && c + 1 < dim ? at + 1 : 0];
            return u32x4_v{a.x, a.y, b.x, b.y};
        }
    }
    return reinterpret_cast<const u32x4_v*>(x)[valid ? at / kBlkE<X> : 0];
}

// w[c .. c + E) as doubles, +0.0 from column dim on and for a lane without a group: element loads.
template <typename W, int E>
__device__ __forceinline__ void blk_load_w_masked(const W* __restrict__ w, int64_t c, int64_t dim, bool valid, double (&wv)[E]) {
#pragma unroll
    for (int e = 0; e < E; e++) {
        const bool on = valid && c + e < dim;
        const double v = (double)w[on ? c + e : 0];
        wv[e] = on ? v : 0.0;
    }
}

// w[c .. c + E) as doubles by 16-byte loads (one 8-byte load for two floats): c + E <= dim, w 16-byte aligned.
template <typename W, int E>
__device__ __forceinline__ void blk_load_w_vec(const W* __restrict__ w, int64_t c, double (&wv)[E]) {
    W t[E];
    if constexpr (E * sizeof(W) == 8) {
        const uint2 a = *reinterpret_cast<const uint2*>(w + c);
        __builtin_memcpy(t, &a, 8);
    } else {
        const u32x4_v* p = reinterpret_cast<const u32x4_v*>(w + c);
#pragma unroll
        for (int i = 0; i < (int)(E * sizeof(W) / 16); i++) {
            const u32x4_v a = p[i];
            __builtin_memcpy(reinterpret_cast<char*>(t) + 16 * i, &a, 16);
        }
    }
#pragma unroll
    for (int e = 0; e < E; e++) wv[e] = (double)t[e];
}

// acc = fma(x[e], w[e], acc) for e = 0 .. E - 1; with MASK an element from column dim on (or of a lane without
// a group) enters as +0.0, whatever the load returned.
template <typename X, bool MASK>
__device__ __forceinline__ void blk_chain(double& acc, const u32x4_v& g, const double (&wv)[kBlkE<X>], int64_t c, int64_t dim, bool valid) {
    double v[kBlkE<X>];
    blk_widen_group<X>(g, v);
#pragma unroll
    for (int e = 0; e < kBlkE<X>; e++) {
        const double xe = !MASK || (valid && c + e < dim) ? v[e] : 0.0;
        acc = __builtin_fma(xe, wv[e], acc);
    }
}

// The sum over the L lanes of a row: a butterfly from L / 2 down to 1; every lane of the group ends with the
// same bits (each step adds the same two values in both lanes).
__device__ __forceinline__ double blk_lane_sum(double v, int lanes) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        if (off < lanes) v += __shfl_xor(v, off);
    return v;
}

template <int LOSS>
__device__ __forceinline__ void blk_finish_row(double acc, const double* __restrict__ label, const GlmWindow& win, int64_t j,
                                               double* __restrict__ pre, double* __restrict__ coef, double* __restrict__ loss) {
    double l, g;
    glm_loss<LOSS>(acc, label[glm_row_of(win, j)], l, g);
    if (pre) pre[j] = acc;
    coef[j] = -1.0 * g;
    if (loss) loss[j] = l;
}

// blockDim.x = 64 * kBlkTeamWaves (split = 1) or 64 * split; see the head of the file.  fast: x and w are both
// read by 16-byte loads (wave-uniform, as lanes and split are).
template <typename X, typename W, int LOSS>
__global__ __launch_bounds__(64 * kBlkMaxSplit) void k_glm_dense_blocked_predict(
    const X* __restrict__ x, const double* __restrict__ label, int64_t dim, int64_t pitch, GlmWindow win, int64_t batch,
    const W* __restrict__ w, int lanes, int split, int x16, int w16, double* __restrict__ pre, double* __restrict__ coef,
    double* __restrict__ loss) {
    constexpr int E = kBlkE<X>;
    __shared__ double s_part[kBlkMaxSplit];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (dim <= (int64_t)64 * E) {  // uniform over the grid
        // ---- short rows: one wave a team, 64 / lanes rows per load instruction, the lane's group of w in registers ----
        const int64_t tm = (int64_t)blockIdx.x * kBlkTeamWaves + wave;
        const int gl = lane % lanes;
        const int64_t c = (int64_t)gl * E;
        const bool colin = c < dim;
        double wv[E];
        blk_load_w_masked<W, E>(w, c, dim, colin, wv);
        for (int step = 0; step < kBlkShortSteps; step++) {
            int64_t j[kBlkRowUnroll];
            u32x4_v g[kBlkRowUnroll];
#pragma unroll
            for (int u = 0; u < kBlkRowUnroll; u++) {
                j[u] = blk_short_row(tm, step, u, lanes, lane);
                const bool valid = colin && j[u] < batch;
                g[u] = blk_load_group<X>(x, valid ? glm_row_of(win, j[u]) * pitch + c : 0, c, dim, x16, valid);
            }
#pragma unroll
            for (int u = 0; u < kBlkRowUnroll; u++) {
                double acc = 0.0;
                blk_chain<X, true>(acc, g[u], wv, c, dim, colin && j[u] < batch);
                acc = blk_lane_sum(acc, lanes);
                if (gl == 0 && j[u] < batch) blk_finish_row<LOSS>(acc, label, win, j[u], pre, coef, loss);
            }
        }
        return;
    }
    // ---- long rows: the `split` waves of a team share batch position tm ----
    const int tpg = split > 1 ? 1 : kBlkTeamWaves;
    const int64_t tm = (int64_t)blockIdx.x * tpg + (split > 1 ? 0 : wave);
    const int s = split > 1 ? wave : 0;
    const bool has = tm < batch;  // wave-uniform
    double acc[kBlkRowUnroll];
#pragma unroll
    for (int q = 0; q < kBlkRowUnroll; q++) acc[q] = 0.0;
    if (has) {
        const int64_t row_at = glm_row_of(win, tm) * pitch;
        const int64_t groups = blk_ceil_div(dim, E), whole = dim / E, stride = blk_long_stride(split);
        const bool fast = x16 && w16;
        for (int64_t base = 0; base < groups; base += stride) {
            u32x4_v g[kBlkRowUnroll];
            double wv[kBlkRowUnroll][E];
            int mode[kBlkRowUnroll];  // wave-uniform per slot: 2 the wave's 64 groups are whole, 1 some exist, 0 none does
#pragma unroll
            for (int q = 0; q < kBlkRowUnroll; q++) {
                const int64_t first = blk_long_group(base, q, split, s, 0), c = (first + lane) * E;
                mode[q] = fast && first + 64 <= whole ? 2 : first < groups ? 1 : 0;
                if (mode[q] == 2) {
                    g[q] = reinterpret_cast<const u32x4_v*>(x)[(row_at + c) / E];
                    blk_load_w_vec<W, E>(w, c, wv[q]);
                } else if (mode[q] == 1) {
                    g[q] = blk_load_group<X>(x, c < dim ? row_at + c : 0, c, dim, x16, c < dim);
                    blk_load_w_masked<W, E>(w, c, dim, c < dim, wv[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < kBlkRowUnroll; q++) {
                const int64_t c = blk_long_group(base, q, split, s, lane) * E;
                if (mode[q] == 2) blk_chain<X, false>(acc[q], g[q], wv[q], c, dim, true);
                else if (mode[q] == 1) blk_chain<X, true>(acc[q], g[q], wv[q], c, dim, c < dim);
            }
        }
    }
    static_assert(kBlkRowUnroll == 4, "the slots are added as (0 + 1) + (2 + 3)");
    double sum = blk_lane_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), 64);
    if (split > 1) {  // uniform over the grid: every wave of the workgroup reaches the barrier
        if (lane == 0) s_part[wave] = sum;
        __syncthreads();
        sum = 0.0;
        for (int i = 0; i < split; i++) sum += s_part[i];
    }
    if (has && threadIdx.x == (split > 1 ? 0 : wave * 64)) blk_finish_row<LOSS>(sum, label, win, tm, pre, coef, loss);
}

// The V columns of one 8-byte load as doubles.
template <typename X>
__device__ __forceinline__ void blk_widen_qword(const uint2& q, double (&v)[kBlkColBytes / (int)sizeof(X)]) {
    if constexpr (std::is_same<X, double>::value) {
        v[0] = __hiloint2double((int)q.y, (int)q.x);
    } else if constexpr (std::is_same<X, float>::value) {
        v[0] = (double)__uint_as_float(q.x);
        v[1] = (double)__uint_as_float(q.y);
    } else {
        float a, b, c, d;
        widen2<X>(q.x, a, b);
        widen2<X>(q.y, c, d);
        v[0] = (double)a;
        v[1] = (double)b;
        v[2] = (double)c;
        v[3] = (double)d;
    }
}

// out: partial (nb > 1; block b's dim sums at b * dim) or g itself (nb = 1, counted into *count).  A lane whose
// first column lies past dim loads the row's first 8 bytes and stores nothing; the chain of a pad column beside
// a last column is never stored or counted.  gridDim = (strips / kBlkColWaves, nb).
template <typename X>
__global__ __launch_bounds__(64 * kBlkColWaves) void k_glm_dense_blocked_partial(
    const X* __restrict__ x, int64_t dim, int64_t pitch, GlmWindow win, int64_t batch, const double* __restrict__ coef, BlkPlan plan,
    double* __restrict__ out, unsigned long long* count) {
    constexpr int XB = (int)sizeof(X), V = kBlkColBytes / XB;
    __shared__ unsigned long long s_cnt;
    const uint2* xq = reinterpret_cast<const uint2*>(x);
    const int lane = threadIdx.x & 63;
    const int64_t strip = (int64_t)blockIdx.x * kBlkColWaves + (threadIdx.x >> 6), b = blockIdx.y;
    const int64_t k0 = blk_col_of<XB>(strip, lane);
    const int64_t q = k0 < dim ? k0 / V : 0;  // the 8-byte word of the row the lane loads
    const int64_t row_q = pitch / V;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; v++) acc[v] = 0.0;
    if (blk_col_of<XB>(strip, 0) < dim) {  // wave-uniform
        int64_t j, j1;
        blk_block_rows(plan, batch, b, &j, &j1);
        for (; j + kBlkU <= j1; j += kBlkU) {
            uint2 xv[kBlkU];
            if (blk_step_contiguous(win, j)) {  // wave-uniform
                const uint2* at = xq + glm_row_of(win, j) * row_q + q;
#pragma unroll
                for (int u = 0; u < kBlkU; u++) xv[u] = at[u * row_q];
            } else {
#pragma unroll
                for (int u = 0; u < kBlkU; u++) xv[u] = xq[glm_row_of(win, j + u) * row_q + q];
            }
#pragma unroll
            for (int u = 0; u < kBlkU; u++) {
                const double c = coef[j + u];
                double e[V];
                blk_widen_qword<X>(xv[u], e);
#pragma unroll
                for (int v = 0; v < V; v++) acc[v] = __builtin_fma(e[v], c, acc[v]);
            }
        }
        for (; j < j1; j++) {  // the last rows of the window's last block: an exact trip count
            const double c = coef[j];
            double e[V];
            blk_widen_qword<X>(xq[glm_row_of(win, j) * row_q + q], e);
#pragma unroll
            for (int v = 0; v < V; v++) acc[v] = __builtin_fma(e[v], c, acc[v]);
        }
    }
    if (plan.nb == 1) {  // uniform over the grid
        LiveCount lc;
#pragma unroll
        for (int v = 0; v < V; v++) {
            const bool on = k0 + v < dim;
            if (on) out[k0 + v] = acc[v];
            lc.add(on && fabs(acc[v]) > 1e-8);  // DenseDoubleGradient.countNNZ
        }
        lc.finish(&s_cnt, count);
    } else {
#pragma unroll
        for (int v = 0; v < V; v++)
            if (k0 + v < dim) out[b * dim + k0 + v] = acc[v];
    }
}

// g[k] = +0.0, then partial[b][k] added for b = 0 .. nb - 1; count += #{|g[k]| > 1e-8}.
__global__ __launch_bounds__(256) void k_glm_dense_blocked_reduce(const double* __restrict__ partial, int64_t dim, int64_t nb,
                                                                  double* __restrict__ g, unsigned long long* count) {
    __shared__ unsigned long long s_cnt;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool on = k < dim;
    double acc = 0.0;
    if (on) {
#pragma unroll 8
        for (int64_t b = 0; b < nb; b++) acc += partial[b * dim + k];
        g[k] = acc;
    }
    LiveCount lc;
    lc.add(on && fabs(acc) > 1e-8);
    lc.finish(&s_cnt, count);
}

// ---- launchers ----
static int blk_x_bytes(int x_kind) { return x_kind == kBlkXF64 ? 8 : x_kind == SKML_X_F32 ? 4 : x_kind == SKML_X_BF16 || x_kind == SKML_X_F16 ? 2 : 0; }

// f(X{}) for the storage type of d.x.
template <typename F>
static hipError_t blk_by_kind(int x_kind, F f) {
    switch (x_kind) {
        case kBlkXF64: return f(double{});
        case SKML_X_F32: return f(float{});
        case SKML_X_BF16: return f(bf16_t{});
        case SKML_X_F16: return f(f16_t{});
        default: return hipErrorInvalidValue;
    }
}

// What the two launches check again: the struct as its entry left it, and the window.
static bool blk_ok(const GlmBlockedX& d, int64_t row0, int64_t batch, BlkPlan* plan) {
    const int xb = blk_x_bytes(d.x_kind);
    if (!xb || !d.x || d.rows < 1 || d.pitch < d.dim || (d.pitch * xb) % 8 || ((uintptr_t)d.x) % 8) return false;
    if (xb != 8 && ((d.pitch * xb) % 16 || ((uintptr_t)d.x) % 16)) return false;
    return batch <= d.rows && row0 >= 0 && row0 < d.rows && blk_plan(xb, batch, d.dim, plan);
}

template <typename X, typename W>
static hipError_t launch_blk_predict_xw(hipStream_t st, const GlmBlockedX& d, const GlmWindow& win, int64_t batch, const BlkPlan& plan,
                                        int loss_kind, const W* w, double* pre, double* coef, double* loss) {
    const int tpg = blk_teams_per_group(plan);
    const dim3 grid((unsigned)blk_ceil_div(blk_teams(plan, batch), tpg)), block(64 * (plan.split > 1 ? plan.split : kBlkTeamWaves));
    const X* x = static_cast<const X*>(d.x);
    const int x16 = (d.pitch * (int64_t)sizeof(X)) % 16 == 0 && ((uintptr_t)d.x) % 16 == 0, w16 = ((uintptr_t)w) % 16 == 0;
    switch (loss_kind) {
        case SKML_LOSS_L1_LOG:
        case SKML_LOSS_L2_LOG:
            hipLaunchKernelGGL((k_glm_dense_blocked_predict<X, W, kGlmLog>), grid, block, 0, st, x, d.label, d.dim, d.pitch, win, batch, w,
                               plan.lanes, plan.split, x16, w16, pre, coef, loss);
            break;
        case SKML_LOSS_L2_HINGE:
            hipLaunchKernelGGL((k_glm_dense_blocked_predict<X, W, kGlmHinge>), grid, block, 0, st, x, d.label, d.dim, d.pitch, win, batch, w,
                               plan.lanes, plan.split, x16, w16, pre, coef, loss);
            break;
        case SKML_LOSS_L2_SQUARE:
            hipLaunchKernelGGL((k_glm_dense_blocked_predict<X, W, kGlmSquare>), grid, block, 0, st, x, d.label, d.dim, d.pitch, win, batch, w,
                               plan.lanes, plan.split, x16, w16, pre, coef, loss);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_glm_dense_blocked_predict(hipStream_t st, const GlmBlockedX& d, int64_t row0, int64_t batch, int loss_kind,
                                            const void* w, int wide, double* pre, double* coef, double* loss) {
    BlkPlan plan;
    if (!blk_ok(d, row0, batch, &plan) || !w || !coef || !d.label) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    return blk_by_kind(d.x_kind, [&](auto xt) {
        using X = decltype(xt);
        return wide ? launch_blk_predict_xw<X>(st, d, win, batch, plan, loss_kind, static_cast<const double*>(w), pre, coef, loss)
                    : launch_blk_predict_xw<X>(st, d, win, batch, plan, loss_kind, static_cast<const float*>(w), pre, coef, loss);
    });
}

hipError_t launch_glm_dense_blocked_plus_by(hipStream_t st, const GlmBlockedX& d, int64_t row0, int64_t batch, const double* coef,
                                            double* partial, double* g, unsigned long long* count) {
    BlkPlan plan;
    if (!blk_ok(d, row0, batch, &plan) || !coef || !g || !count || (plan.nb > 1 && !partial)) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    const hipError_t e = blk_by_kind(d.x_kind, [&](auto xt) {
        using X = decltype(xt);
        const int64_t strips = blk_strips<(int)sizeof(X)>(d.dim);
        const dim3 grid((unsigned)blk_ceil_div(strips, kBlkColWaves), (unsigned)plan.nb);
        hipLaunchKernelGGL(k_glm_dense_blocked_partial<X>, grid, dim3(64 * kBlkColWaves), 0, st, static_cast<const X*>(d.x), d.dim,
                           d.pitch, win, batch, coef, plan, plan.nb > 1 ? partial : g, count);
        return hipGetLastError();
    });
    if (e != hipSuccess || plan.nb == 1) return e;
    hipLaunchKernelGGL(k_glm_dense_blocked_reduce, dim3((unsigned)blk_ceil_div(d.dim, 256)), dim3(256), 0, st, partial, d.dim, plan.nb, g,
                       count);
    return hipGetLastError();
}

}  // namespace skml
