// skml_glm_dense_multi.hip -- the mini-batch gradient over dense instances for K <= 16 models in one pass over x:
// the GEMM-shaped variant of the blocked order (skml_glm_dense_blocked.hip) on v_mfma_f64_16x16x4_f64.  K calls
// of the blocked entries read the same window of x K times and are bound by those bytes; here the row dot is
// pre = X . W^T (16 window rows x 16 models per accumulator) and the column sum is G = Coef^T . X (16 models x 16
// columns per accumulator), so x is read twice whatever K is.  One source for the four storages of x (double,
// fp32, bf16, fp16) and both weight types.
//
// The contract.  All arithmetic is in double; a narrow x is widened exactly.  Every sum starts from +0.0 and
// there is no floating-point atomic (the only atomics are the integer ones of the live counts).  The order of
// every sum is a function of batch, dim, K, the storage type and the constants of skml_glm_dense_multi.hpp (row0
// enters only through the window), so the same call gives the same bits on every run.  The order in which the
// instruction adds its own four products is the hardware's: fixed, not specified here, and so no bit parity
// with the blocked or the sequential order is claimed, only the error bound of any order.  coef, loss, objLoss
// and toAuto's count come from this pre and this grad as in the blocked entries (glm_loss, the fixed-shape loss
// sum per model, LiveCount's test).  NaN and Inf take part as in any IEEE sum.  A lane that stands for a row past
// batch, a column past dim (pad elements of a pitched row included) or a model past K loads nothing for it and
// feeds +0.0: the instruction multiplies +0.0 by +0.0 there (or by a finite or non-finite value of the other
// operand only where that product belongs to an output that is never stored).
//
// The instruction (CDNA3 / CDNA4 ISA, "V_MFMA_F64_16X16X4_F64"): D(16 x 16) = A(16 x 4) . B(4 x 16) + C; lane l
// holds A[l % 16][l / 16] and B[l / 16][l % 16], one double each, and D[4 * r + l / 16][l % 16] in register
// pair r = 0 .. 3 (the integer tests pin this layout: any other permutes rows or models).  The k index (l / 16) is a free permutation as long as both operands use the same one.
//
//   k_glm_dense_multi_predict<X, W, LOSS, R>  a wave owns R tiles of 16 window rows and walks dim.  A = x: lane
//       (row i = l % 16, slot q = l / 16) loads the E = 16 / sizeof(X) consecutive columns (step * 4 + q) * E + e
//       of its row by one 16-byte load and feeds them to E instructions in turn; B = w: lane (model m = l % 16,
//       slot q) loads the same E columns of model m.  A wave-load of x is 16 rows x 64 contiguous bytes.  Latency:
//       the instruction occupies the matrix pipe for 8 passes and a dependent one cannot issue back to back, so
//       a wave keeps kMulAcc = 4 independent accumulators: R = 4 row tiles that share one load of w (many rows),
//       or R = 1 tile, 2 wave-steps in flight and one accumulator each for a lane's even and odd columns (few
//       rows), added as (0 + 1) + (2 + 3).  With too few tiles for
//       the device (R = 1) dim is split over the S waves of a workgroup; their accumulators meet in LDS and are
//       added in wave order from +0.0.  Epilogue: every lane holds four (row, model) sums, applies glm_loss to
//       them against its model's labels and stores pre, coef and loss model-major.
//   k_glm_dense_multi_partial<X>              grid = column strips x NB row blocks.  B = x: lane (column n = l % 16,
//       row slot k = l / 16) loads kMulWords 8-byte words of row j + k, 16 lanes apart, and spreads their
//       V = 8 / sizeof(X) columns over kMulWords * V accumulator tiles; A = coef: lane (model m, slot k) loads
//       coef[m][j + k].  kMulU steps of 4 rows have their loads in flight ahead of the MFMAs.  Block b stores
//       partial[b][K][dim]; with NB = 1 it stores grad itself and counts.
//   k_glm_dense_multi_reduce                  a lane per (model, column) adds the NB partials in block order from
//       +0.0, stores grad and feeds that model's LiveCount.
//   k_glm_dense_multi_loss_sum                k_glm_loss_sum's fixed shape, one workgroup per model.
// Packed fp32 arithmetic: nothing here computes in fp32 (floats are only converted, by v_cvt_f64_f32 and
// v_cvt_f32_f16, which have no packed form that the compiler selects), so this file builds with the default
// target features; the disassembly holds no v_pk_* instruction.
#include "skml_device.hpp"
#include "skml_glm_dense_multi.hpp"
#include "skml_glm_device.hpp"
#include "skml_opt.hpp"

namespace skml {

typedef double f64x4_v __attribute__((ext_vector_type(4)));

template <typename X>
constexpr int kMulE = 16 / (int)sizeof(X);

__device__ __forceinline__ f64x4_v mul_mfma(double a, double b, const f64x4_v& c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// The E values of one 16-byte group as doubles, exactly.
template <typename X>
__device__ __forceinline__ void mul_widen_group(const u32x4_v& g, double (&v)[kMulE<X>]) {
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

// The V values of one 8-byte word as doubles, exactly.
template <typename X>
__device__ __forceinline__ void mul_widen_word(const uint2& q, double (&v)[8 / (int)sizeof(X)]) {
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

// The group of E elements at element `at` of x, whose first column is c < dim; all-zero bits (E times +0.0)
// without a load when !valid.  x16: rows start on 16-byte boundaries (always for a narrow x: the pitch rule);
// otherwise x holds doubles and each is loaded alone, the second only where the row has it.
template <typename X>
__device__ __forceinline__ u32x4_v mul_load_group(const X* __restrict__ x, int64_t at, int64_t c, int64_t dim, bool x16, bool valid) {
    u32x4_v g = {0u, 0u, 0u, 0u};
    if (valid) {
        if constexpr (std::is_same<X, double>::value) {
            if (!x16) {
                const uint2* xq = reinterpret_cast<const uint2*>(x);
                const uint2 a = xq[at];
                g.x = a.x;
                g.y = a.y;
                if (c + 1 < dim) {
                    const uint2 b = xq[at + 1];
                    g.z = b.x;
                    g.w = b.y;
                }
                return g;
            }
        }
        g = reinterpret_cast<const u32x4_v*>(x)[at / kMulE<X>];
    }
    return g;
}

// w[at + e] as doubles for the columns c + e < dim of a lane with a model (`on`), +0.0 elsewhere: element loads.
template <typename W, int E>
__device__ __forceinline__ void mul_load_w_masked(const W* __restrict__ w, int64_t at, int64_t c, int64_t dim, bool on, double (&wv)[E]) {
#pragma unroll
    for (int e = 0; e < E; e++) wv[e] = on && c + e < dim ? (double)w[at + e] : 0.0;
}

// w[at .. at + E) as doubles by 16-byte loads (one 8-byte load for two floats) for a lane with a model, +0.0
// without: the E columns exist and w + at is aligned to the load.
template <typename W, int E>
__device__ __forceinline__ void mul_load_w_vec(const W* __restrict__ w, int64_t at, bool on, double (&wv)[E]) {
    W t[E];
#pragma unroll
    for (int e = 0; e < E; e++) t[e] = (W)0;
    if (on) {
        if constexpr (E * sizeof(W) == 8) {
            const uint2 a = *reinterpret_cast<const uint2*>(w + at);
            __builtin_memcpy(t, &a, 8);
        } else {
            const u32x4_v* p = reinterpret_cast<const u32x4_v*>(w + at);
#pragma unroll
            for (int i = 0; i < (int)(E * sizeof(W) / 16); i++) {
                const u32x4_v a = p[i];
                __builtin_memcpy(reinterpret_cast<char*>(t) + 16 * i, &a, 16);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; e++) wv[e] = (double)t[e];
}

// blockDim.x = 64 * kMulTeamWaves (split = 1) or 64 * split (R = 1 only); see the head of the file.  labels: K x rows
// model-major, or null: every model takes label.  fast: x and w are both read by 16-byte loads.
template <typename X, typename W, int LOSS, int R>
__global__ __launch_bounds__(64 * kMulMaxSplit) void k_glm_dense_multi_predict(
    const X* __restrict__ x, const double* __restrict__ label, const double* __restrict__ labels, int64_t rows, int64_t dim, int64_t pitch,
    GlmWindow win, int64_t batch, const W* __restrict__ w, int models, int split, int x16, int w16, double* __restrict__ pre,
    double* __restrict__ coef, double* __restrict__ loss) {
    constexpr int E = kMulE<X>, CS = mul_steps_in_flight(R), P = kMulAcc / (R * CS);
    static_assert(R == 1 || R == kMulAcc, "four tiles that share w, or one tile, two wave-steps in flight and two accumulators each");
    __shared__ double s_part[R == 1 ? kMulMaxSplit : 1][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int64_t team = split > 1 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kMulTeamWaves + wave;
    const int s = split > 1 ? wave : 0;
    const int64_t tile0 = team * R;
    const bool has = tile0 < mul_tiles(batch);  // wave-uniform
    f64x4_v acc[R][CS][P];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int a = 0; a < CS; a++)
#pragma unroll
            for (int p = 0; p < P; p++) acc[r][a][p] = f64x4_v{0.0, 0.0, 0.0, 0.0};
    if (has) {
        int64_t row_at[R];
        bool row_on[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int64_t j = (tile0 + r) * kMulTileRows + i;
            row_on[r] = j < batch;
            row_at[r] = row_on[r] ? glm_row_of(win, j) * pitch : 0;
        }
        const bool w_on = i < models;
        const int64_t w_at = w_on ? (int64_t)i * dim : 0;
        const int64_t steps = mul_col_steps(E, dim), stride = (int64_t)CS * split;
        const bool fast = x16 && w16;
        for (int64_t base = 0; base < steps; base += stride) {
            u32x4_v g[R][CS];
            double wv[CS][E];
            int mode[CS];  // wave-uniform per wave-step: 2 its columns all exist, 1 some do, 0 no such wave-step
#pragma unroll
            for (int a = 0; a < CS; a++) {
                const int64_t step = mul_step_of(base, a, split, s), c = mul_lane_col(step, q, E);
                mode[a] = step >= steps ? 0 : fast && (step + 1) * kMulK * E <= dim ? 2 : 1;
                if (mode[a] == 2) {
#pragma unroll
                    for (int r = 0; r < R; r++) g[r][a] = mul_load_group<X>(x, row_at[r] + c, c, dim, true, row_on[r]);
                    mul_load_w_vec<W, E>(w, w_at + c, w_on, wv[a]);
                } else {
#pragma unroll
                    for (int r = 0; r < R; r++) g[r][a] = mul_load_group<X>(x, row_at[r] + c, c, dim, x16, mode[a] == 1 && row_on[r] && c < dim);
                    mul_load_w_masked<W, E>(w, w_at + c, c, dim, mode[a] == 1 && w_on, wv[a]);
                }
            }
#pragma unroll
            for (int a = 0; a < CS; a++) {
                // a wave-step past the row's last feeds +0.0 x +0.0 to accumulators that started at +0.0 and only add: no bit changes
                const int64_t c = mul_lane_col(mul_step_of(base, a, split, s), q, E);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    double v[E];
                    mul_widen_group<X>(g[r][a], v);
#pragma unroll
                    for (int e = 0; e < E; e++) {
                        // a pad element beside the row's last column was loaded: +0.0 in its place
                        const double xe = mode[a] == 2 || c + e < dim ? v[e] : 0.0;
                        acc[r][a][e % P] = mul_mfma(xe, wv[a][e], acc[r][a][e % P]);
                    }
                }
            }
        }
    }
    f64x4_v sum[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        if constexpr (R == 1) sum[r] = (acc[r][0][0] + acc[r][0][1]) + (acc[r][1][0] + acc[r][1][1]);
        else sum[r] = acc[r][0][0];
    }
    if constexpr (R == 1) {
        if (split > 1) {  // uniform over the grid: every wave of the workgroup reaches the barrier
#pragma unroll
            for (int rr = 0; rr < 4; rr++) s_part[wave][rr * 64 + lane] = sum[0][rr];
            __syncthreads();
            if (wave != 0) return;
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                double t = 0.0;
                for (int k = 0; k < split; k++) t += s_part[k][rr * 64 + lane];
                sum[0][rr] = t;
            }
        }
    }
    if (!has || i >= models) return;
    // D layout: this lane holds model i and the rows 4 rr + q of each of its tiles
    const double* y = labels ? labels + (int64_t)i * rows : label;
    const int64_t out_at = (int64_t)i * batch;
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int64_t j = mul_out_row(tile0 + r, lane, rr);
            if (j >= batch) continue;
            double l, gr;
            glm_loss<LOSS>(sum[r][rr], y[glm_row_of(win, j)], l, gr);
            if (pre) pre[out_at + j] = sum[r][rr];
            coef[out_at + j] = -1.0 * gr;
            if (loss) loss[out_at + j] = l;
        }
}

// out: partial (nb > 1; block b's K x dim sums at b * K * dim) or grad itself (nb = 1, counted into count[model]).
// coef: K x batch, model-major.  gridDim = (strips / kMulColWaves, nb).
template <typename X>
__global__ __launch_bounds__(64 * kMulColWaves) void k_glm_dense_multi_partial(
    const X* __restrict__ x, int64_t dim, int64_t pitch, GlmWindow win, int64_t batch, const double* __restrict__ coef, int models,
    MulPlan plan, double* __restrict__ out, unsigned long long* count) {
    constexpr int XB = (int)sizeof(X), V = 8 / XB, T = kMulWords;
    __shared__ unsigned long long s_cnt[kMulMaxModels];
    const uint2* xq = reinterpret_cast<const uint2*>(x);
    const int lane = threadIdx.x & 63, n = lane & 15, k = lane >> 4;
    const int64_t strip = (int64_t)blockIdx.x * kMulColWaves + (threadIdx.x >> 6), b = blockIdx.y;
    const int64_t row_q = pitch / V;
    int64_t c0[T], word[T];
    bool col_on[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
        c0[t] = mul_col_of<XB>(strip, t, n);
        col_on[t] = c0[t] < dim;
        word[t] = col_on[t] ? c0[t] / V : 0;
    }
    f64x4_v acc[T][V];
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int v = 0; v < V; v++) acc[t][v] = f64x4_v{0.0, 0.0, 0.0, 0.0};
    if (mul_col_of<XB>(strip, 0, 0) < dim) {  // wave-uniform
        int64_t j0, j1;
        mul_block_rows(plan, batch, b, &j0, &j1);
        const bool m_on = n < models;
        const double* cf = coef + (m_on ? (int64_t)n * batch : 0);
        const bool whole_cols = mul_col_of<XB>(strip + 1, 0, 0) <= dim;  // wave-uniform: no column of the strip is masked
        for (int64_t j = j0; j < j1; j += kMulRowsPerIter) {
            uint2 xv[kMulU][T];
            double cv[kMulU];
#pragma unroll
            for (int u = 0; u < kMulU; u++) {
                const int64_t jj = mul_row_pos(j, u, k);
                const bool on = jj < j1;
                const int64_t at = on ? glm_row_of(win, jj) * row_q : 0;
#pragma unroll
                for (int t = 0; t < T; t++) {
                    xv[u][t] = uint2{0u, 0u};
                    if (on && col_on[t]) xv[u][t] = xq[at + word[t]];
                }
                cv[u] = 0.0;
                if (on && m_on) cv[u] = cf[jj];
            }
#pragma unroll
            for (int u = 0; u < kMulU; u++)
#pragma unroll
                for (int t = 0; t < T; t++) {
                    double e[V];
                    mul_widen_word<X>(xv[u][t], e);
                    if (!whole_cols) {  // a pad element beside the row's last column was loaded: +0.0 in its place
#pragma unroll
                        for (int v = 0; v < V; v++) e[v] = c0[t] + v < dim ? e[v] : 0.0;
                    }
#pragma unroll
                    for (int v = 0; v < V; v++) acc[t][v] = mul_mfma(cv[u], e[v], acc[t][v]);
                }
        }
    }
    // D layout: this lane holds the models 4 r + k of column c0[t] + v
    const bool direct = plan.nb == 1;  // uniform over the grid
    if (direct) {
        if (threadIdx.x < kMulMaxModels) s_cnt[threadIdx.x] = 0;
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int m = mul_out_model(lane, r);
        if (m >= models) continue;
        double* o = out + (direct ? (int64_t)m : b * models + m) * dim;
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int v = 0; v < V; v++) {
                if (c0[t] + v >= dim) continue;
                o[c0[t] + v] = acc[t][v][r];
                if (direct && fabs(acc[t][v][r]) > 1e-8) atomicAdd(&s_cnt[m], 1ull);  // DenseDoubleGradient.countNNZ
            }
    }
    if (direct) {
        __syncthreads();
        if ((int)threadIdx.x < models && s_cnt[threadIdx.x]) atomicAdd(&count[threadIdx.x], s_cnt[threadIdx.x]);
    }
}

// g[m][k] = +0.0, then partial[b][m][k] added for b = 0 .. nb - 1; count[m] += #{|g[m][k]| > 1e-8}.  gridDim.y = K.
__global__ __launch_bounds__(256) void k_glm_dense_multi_reduce(const double* __restrict__ partial, int64_t dim, int64_t nb, int models,
                                                                double* __restrict__ g, unsigned long long* count) {
    __shared__ unsigned long long s_cnt;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    const bool on = k < dim;
    double acc = 0.0;
    if (on) {
#pragma unroll 8
        for (int64_t b = 0; b < nb; b++) acc += partial[(b * models + m) * dim + k];
        g[m * dim + k] = acc;
    }
    LiveCount lc;
    lc.add(on && fabs(acc) > 1e-8);
    lc.finish(&s_cnt, count + m);
}

// k_glm_loss_sum's shape per model: thread t adds loss[m][t], loss[m][t + 1024], ... from +0.0, then the 1024 sums
// meet in a binary tree.  gridDim.x = K.
__global__ __launch_bounds__(1024) void k_glm_dense_multi_loss_sum(const double* __restrict__ loss, int64_t n, double* __restrict__ obj) {
    __shared__ double s[1024];
    const double* l = loss + (int64_t)blockIdx.x * n;
    double a = 0.0;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < n; i += 1024) a += l[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) obj[blockIdx.x] = s[0];
}

// ---- launchers ----
static int mul_x_bytes(int x_kind) { return x_kind == kBlkXF64 ? 8 : x_kind == SKML_X_F32 ? 4 : x_kind == SKML_X_BF16 || x_kind == SKML_X_F16 ? 2 : 0; }

// f(X{}) for the storage type of d.x.
template <typename F>
static hipError_t mul_by_kind(int x_kind, F f) {
    switch (x_kind) {
        case kBlkXF64: return f(double{});
        case SKML_X_F32: return f(float{});
        case SKML_X_BF16: return f(bf16_t{});
        case SKML_X_F16: return f(f16_t{});
        default: return hipErrorInvalidValue;
    }
}

// What the launches check again: the struct as its entry left it, the window and K.
static bool mul_ok(const GlmBlockedX& d, int64_t row0, int64_t batch, int models, MulPlan* plan) {
    const int xb = mul_x_bytes(d.x_kind);
    if (!xb || !d.x || d.rows < 1 || d.pitch < d.dim || (d.pitch * xb) % 8 || ((uintptr_t)d.x) % 8) return false;
    if (xb != 8 && ((d.pitch * xb) % 16 || ((uintptr_t)d.x) % 16)) return false;
    return batch <= d.rows && row0 >= 0 && row0 < d.rows && mul_plan(xb, models, batch, d.dim, plan);
}

template <typename X, typename W, int LOSS>
static void launch_mul_predict_l(hipStream_t st, const GlmBlockedX& d, const GlmWindow& win, int64_t batch, const MulPlan& plan,
                                 const W* w, int models, const double* labels, double* pre, double* coef, double* loss) {
    const dim3 grid((unsigned)mul_ceil_div(mul_teams(plan, batch), mul_teams_per_group(plan))),
        block(64 * (plan.split > 1 ? plan.split : kMulTeamWaves));
    const X* x = static_cast<const X*>(d.x);
    const int x16 = (d.pitch * (int64_t)sizeof(X)) % 16 == 0 && ((uintptr_t)d.x) % 16 == 0;
    const int w16 = ((uintptr_t)w) % 16 == 0 && (d.dim * (int64_t)sizeof(W)) % 16 == 0;  // every model's row of w
    if (plan.tiles_per_wave == 1)
        hipLaunchKernelGGL((k_glm_dense_multi_predict<X, W, LOSS, 1>), grid, block, 0, st, x, d.label, labels, d.rows, d.dim, d.pitch, win,
                           batch, w, models, plan.split, x16, w16, pre, coef, loss);
    else
        hipLaunchKernelGGL((k_glm_dense_multi_predict<X, W, LOSS, kMulAcc>), grid, block, 0, st, x, d.label, labels, d.rows, d.dim, d.pitch,
                           win, batch, w, models, plan.split, x16, w16, pre, coef, loss);
}

template <typename X, typename W>
static hipError_t launch_mul_predict_xw(hipStream_t st, const GlmBlockedX& d, const GlmWindow& win, int64_t batch, const MulPlan& plan,
                                        int loss_kind, const W* w, int models, const double* labels, double* pre, double* coef,
                                        double* loss) {
    switch (loss_kind) {
        case SKML_LOSS_L1_LOG:
        case SKML_LOSS_L2_LOG: launch_mul_predict_l<X, W, kGlmLog>(st, d, win, batch, plan, w, models, labels, pre, coef, loss); break;
        case SKML_LOSS_L2_HINGE: launch_mul_predict_l<X, W, kGlmHinge>(st, d, win, batch, plan, w, models, labels, pre, coef, loss); break;
        case SKML_LOSS_L2_SQUARE: launch_mul_predict_l<X, W, kGlmSquare>(st, d, win, batch, plan, w, models, labels, pre, coef, loss); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_glm_dense_multi_predict(hipStream_t st, const GlmBlockedX& d, int64_t row0, int64_t batch, int loss_kind, const void* w,
                                          int wide, int models, const double* labels, double* pre, double* coef, double* loss) {
    MulPlan plan;
    if (!mul_ok(d, row0, batch, models, &plan) || !w || !coef || (!labels && !d.label)) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    return mul_by_kind(d.x_kind, [&](auto xt) {
        using X = decltype(xt);
        return wide ? launch_mul_predict_xw<X>(st, d, win, batch, plan, loss_kind, static_cast<const double*>(w), models, labels, pre, coef, loss)
                    : launch_mul_predict_xw<X>(st, d, win, batch, plan, loss_kind, static_cast<const float*>(w), models, labels, pre, coef, loss);
    });
}

hipError_t launch_glm_dense_multi_loss_sum(hipStream_t st, const double* loss, int64_t batch, int models, double* obj) {
    if (!loss || !obj || batch < 1 || models < 1 || models > kMulMaxModels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_glm_dense_multi_loss_sum, dim3((unsigned)models), dim3(1024), 0, st, loss, batch, obj);
    return hipGetLastError();
}

hipError_t launch_glm_dense_multi_plus_by(hipStream_t st, const GlmBlockedX& d, int64_t row0, int64_t batch, const double* coef, int models,
                                          double* partial, double* g, unsigned long long* count) {
    MulPlan plan;
    if (!mul_ok(d, row0, batch, models, &plan) || !coef || !g || !count || (plan.nb > 1 && !partial)) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    const hipError_t e = mul_by_kind(d.x_kind, [&](auto xt) {
        using X = decltype(xt);
        const dim3 grid((unsigned)mul_ceil_div(mul_strips((int)sizeof(X), d.dim), kMulColWaves), (unsigned)plan.nb);
        hipLaunchKernelGGL(k_glm_dense_multi_partial<X>, grid, dim3(64 * kMulColWaves), 0, st, static_cast<const X*>(d.x), d.dim, d.pitch,
                           win, batch, coef, models, plan, plan.nb > 1 ? partial : g, count);
        return hipGetLastError();
    });
    if (e != hipSuccess || plan.nb == 1) return e;
    hipLaunchKernelGGL(k_glm_dense_multi_reduce, dim3((unsigned)mul_ceil_div(d.dim, 256), (unsigned)models), dim3(256), 0, st, partial, d.dim,
                       plan.nb, models, g, count);
    return hipGetLastError();
}

}  // namespace skml
