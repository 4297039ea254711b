// skml_glm.hip -- the mini-batch gradient on the device (ml/objective/GradientDescent.scala:23-87,
// ml/objective/Loss.scala:56-137, ml/util/Maths.scala:57-69, DenseDoubleGradient.scala:51-57):
//   k_glm_predict<W, LOSS, LPR>  Maths.dot(w, x_j) per row of the window with 1, 8 or 64 lanes per row
//                                (gathers and products across lanes, the add chain in entry order),
//                                then loss.loss / -1.0 * loss.grad
//   k_glm_loss_sum               sum of loss_j: one workgroup, strided sequential sums, a fixed tree
//   k_glm_valid<W, LOSS, LPR>    the validation pass (ml/util/ValidationUtil.scala:12-41): the same row dot
//                                over every row, loss.loss, the four confusion counts
//   k_glm_seq_sum                sum of n doubles in index order, the reference's bits: one wave
//   k_glm_plus_by                g[k] per column in batch order: a lane for a column with a short
//                                window, the wave for a long one; +0.0 where the window is empty;
//                                toAuto's live count on the way
//   k_glm_finish<W>              timesBy and the regulariser in place, dense or keys + values
// The window split and the ordered column walk are skml_glm.hpp's, shared with tests/glm_check.cpp.
// Every sum starts at +0.0 and only adds, so it never holds -0.0; adding +0.0 for an entry that is
// refused (out of range) therefore changes no bit.
#include <algorithm>

#include "skml_device.hpp"
#include "skml_glm.hpp"
#include "skml_opt.hpp"
#include "skml_valid.hpp"

namespace skml {

constexpr int kGlmLog = 0, kGlmHinge = 1, kGlmSquare = 2;
constexpr int kGlmLaneMax = 32;  // a column with at most this many window entries is summed by its own lane
constexpr int kGlmU = 4;         // chunks of 64 entries the wave form of k_glm_plus_by keeps in flight

// p of lane i (wave-uniform) in every lane.
__device__ __forceinline__ double lane_value64(double p, int i) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(p), i);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(p), i);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int64_t uniform_i64(int64_t x, int src) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)x, src);
    const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)x >> 32), src);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
// acc + p[lane 0] + p[lane 1] + ... + p[lane cnt - 1], one rounded add after the other; cnt is
// wave-uniform in [1, 64] and every lane returns the same sum.
__device__ __forceinline__ double ordered_add64(double acc, double p, int cnt) {
    if (cnt == 64) {
#pragma unroll
        for (int i = 0; i < 64; i++) acc += lane_value64(p, i);
    } else {
        for (int i = 0; i < cnt; i++) acc += lane_value64(p, i);
    }
    return acc;
}

// The same from a wave's LDS slots: acc + s[0] + ... + s[cnt - 1].  Every lane reads the same address
// (a broadcast), and the reads do not depend on the sum, so only the adds form the chain.
__device__ __forceinline__ double ordered_add_lds(double acc, const double* s, int cnt) {
    if (cnt == 64) {
#pragma unroll
        for (int i = 0; i < 64; i++) acc += s[i];
    } else {
        for (int i = 0; i < cnt; i++) acc += s[i];
    }
    return acc;
}

__device__ __forceinline__ int64_t clamp_ptr(int64_t p, int64_t nnz) { return p < 0 ? 0 : (p > nnz ? nnz : p); }

// loss.loss(pre, y) and loss.grad(pre, y), the branches as Loss.scala writes them.  L1LogLoss and
// L2LogLoss share their arithmetic.
template <int LOSS>
__device__ __forceinline__ void glm_loss(double pre, double y, double& loss, double& grad) {
    if constexpr (LOSS == kGlmLog) {
        const double z = pre * y;
        if (z > 18) {
            const double e = exp(-z);
            loss = e;
            grad = y * e;
        } else if (z < -18) {
            loss = -z;
            grad = y;
        } else {
            loss = log(1.0 + exp(-z));
            grad = y / (1.0 + exp(z));
        }
    } else if constexpr (LOSS == kGlmHinge) {
        const double z = pre * y;
        loss = z < 1.0 ? 1.0 - z : 0.0;
        grad = z <= 1.0 ? y : 0.0;
    } else {
        const double d = pre - y;
        loss = (0.5 * d) * d;
        grad = y - pre;
    }
}

// Maths.dot(w, x_row) over the row's entries [s, e) by the row's LPR lanes (sub = the lane's place among
// them): the gathers and products across lanes, the adds one after the other in stored order from
// +0.0.  Every lane of a wave reaches the call (the cross-lane reads need them all); with LPR == 64
// s and e are taken from lane 0.  Every lane of the row returns the sum.
template <typename W, int LPR>
__device__ __forceinline__ double glm_row_dot(const skml_glm_data& d, const W* __restrict__ w, int64_t s, int64_t e,
                                              int sub) {
    double acc = 0.0;
    if constexpr (LPR == 1) {
        for (int64_t i = s; i < e; i++) {
            const int32_t c = d.col[i];
            if ((uint32_t)c >= (uint64_t)d.dim) continue;
            const double p = (double)w[c] * d.val[i];
            acc += p;
        }
    } else if constexpr (LPR == 64) {
        const int64_t us = uniform_i64(s, 0), ue = uniform_i64(e, 0);  // one row per wave
        for (int64_t b = us; b < ue; b += 64) {
            const int64_t i = b + sub;
            double p = 0.0;
            if (i < ue) {
                const int32_t c = d.col[i];
                if ((uint32_t)c < (uint64_t)d.dim) p = (double)w[c] * d.val[i];
            }
            acc = ordered_add64(acc, p, (int)std::min<int64_t>(64, ue - b));
        }
    } else {
        const int64_t len = e - s;
        for (int64_t b = 0; __any(b < len); b += LPR) {
            const int64_t i = s + b + sub;
            double p = 0.0;
            if (i < e) {
                const int32_t c = d.col[i];
                if ((uint32_t)c < (uint64_t)d.dim) p = (double)w[c] * d.val[i];
            }
#pragma unroll
            for (int t = 0; t < LPR; t++) {
                const double q = __shfl(p, t, LPR);
                if (b + t < len) acc += q;
            }
        }
    }
    return acc;
}

template <typename W, int LOSS, int LPR>
__global__ __launch_bounds__(256) void k_glm_predict(skml_glm_data d, GlmWindow win, int64_t batch,
                                                     const W* __restrict__ w, double* __restrict__ pre,
                                                     double* __restrict__ coef, double* __restrict__ loss) {
    constexpr int kRows = 256 / LPR;  // rows per workgroup and step
    const int sub = threadIdx.x % LPR;
    // the trip count is the workgroup's: the cross-lane reads below need every lane of a wave
    for (int64_t jb = (int64_t)blockIdx.x * kRows; jb < batch; jb += (int64_t)gridDim.x * kRows) {
        const int64_t j = jb + threadIdx.x / LPR;
        const bool on = j < batch;
        int64_t row = 0, s = 0, e = 0;
        if (on) {
            row = glm_row_of(win, j);
            s = clamp_ptr(d.row_ptr[row], d.nnz);
            e = clamp_ptr(d.row_ptr[row + 1], d.nnz);
            if (e < s) e = s;
        }
        const double acc = glm_row_dot<W, LPR>(d, w, s, e, sub);
        if (on && sub == 0) {
            double l, g;
            glm_loss<LOSS>(acc, d.label[row], l, g);
            if (pre) pre[j] = acc;
            coef[j] = -1.0 * g;
            if (loss) loss[j] = l;
        }
    }
}

// The validation pass (ml/util/ValidationUtil.scala:21-31) over every row of the data set: the row dot
// of k_glm_predict, loss.loss, and the instance's class.  cnt[0 .. 4) += truePos, trueNeg, falsePos,
// falseNeg and cnt[4] += the NaN scores, as LiveCount counts: a ballot and a popcount per wave, one LDS
// add per wave, one global atomic per workgroup and counter (integer sums: no order to depend on).
// The column-order arrays of d are not read.
constexpr int kValidCounters = 5;
template <typename W, int LOSS, int LPR>
__global__ __launch_bounds__(256) void k_glm_valid(skml_glm_data d, const W* __restrict__ w, double* __restrict__ pre,
                                                   double* __restrict__ loss, unsigned long long* __restrict__ cnt) {
    __shared__ unsigned long long s_cnt[kValidCounters];
    constexpr int kRows = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    unsigned long long wave[kValidCounters] = {0, 0, 0, 0, 0};  // wave-uniform
    // the trip count is the workgroup's: the cross-lane reads and the ballots need every lane of a wave
    for (int64_t jb = (int64_t)blockIdx.x * kRows; jb < d.rows; jb += (int64_t)gridDim.x * kRows) {
        const int64_t row = jb + threadIdx.x / LPR;
        const bool on = row < d.rows;
        int64_t s = 0, e = 0;
        if (on) {
            s = clamp_ptr(d.row_ptr[row], d.nnz);
            e = clamp_ptr(d.row_ptr[row + 1], d.nnz);
            if (e < s) e = s;
        }
        const double acc = glm_row_dot<W, LPR>(d, w, s, e, sub);
        int cls = kValidNone;
        bool nan = false;
        if (on && sub == 0) {
            const double y = d.label[row];
            double l, g;
            glm_loss<LOSS>(acc, y, l, g);
            if (pre) pre[row] = acc;
            loss[row] = l;
            cls = valid_class(acc, y);
            nan = acc != acc;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) wave[k] += (unsigned long long)__popcll(__ballot(cls == k + 1));
        wave[4] += (unsigned long long)__popcll(__ballot(nan));
    }
    if (threadIdx.x < kValidCounters) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kValidCounters; k++)
            if (wave[k]) atomicAdd(&s_cnt[k], wave[k]);
    }
    __syncthreads();
    if (threadIdx.x < kValidCounters && s_cnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
}

// acc = 0.0; for i: acc += x[i], the reference's `validLoss += ...` / `objLoss += ...` bit for bit: a
// chain of n dependent adds, so one wave of one workgroup.  The wave stages kSeqStep values through its
// LDS slots and adds them from broadcast reads while the next kSeqStep are in flight
// (glm_wave_range_sum's pattern; the chunk walk is skml_valid.hpp's).
__device__ __forceinline__ void seq_load(double (&p)[kSeqU], const double* __restrict__ x, int64_t b, int64_t n, int lane) {
#pragma unroll
    for (int u = 0; u < kSeqU; u++) {
        const int64_t i = seq_index(b, u, lane);
        p[u] = i < n ? x[i] : 0.0;
    }
}
__global__ __launch_bounds__(64) void k_glm_seq_sum(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
    __shared__ double slots[kSeqStep];
    const int lane = threadIdx.x;
    double acc = 0.0;
    double nxt[kSeqU];
    seq_load(nxt, x, 0, n, lane);
    for (int64_t b = 0; b < n; b += kSeqStep) {
#pragma unroll
        for (int u = 0; u < kSeqU; u++) slots[u * 64 + lane] = nxt[u];
        if (b + kSeqStep < n) seq_load(nxt, x, b + kSeqStep, n, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < kSeqU; u++) {
            const int cnt = seq_chunk_count(n, b, u);
            if (cnt > 0) acc = ordered_add_lds(acc, slots + u * 64, cnt);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane == 0) *out = acc;
}

// Fixed shape, so the same bits on every run: thread t adds loss[t], loss[t + 1024], ... from +0.0,
// then the 1024 sums meet in a binary tree.
__global__ __launch_bounds__(1024) void k_glm_loss_sum(const double* __restrict__ loss, int64_t n,
                                                       double* __restrict__ obj) {
    __shared__ double s[1024];
    double a = 0.0;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < n; i += 1024) a += loss[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *obj = s[0];
}

// The products of kGlmU chunks of 64 entries from b on, lane by lane; +0.0 past e.
__device__ __forceinline__ void glm_load_products(double (&p)[kGlmU], const int32_t* __restrict__ csc_row,
                                                  const double* __restrict__ csc_val, int64_t b, int64_t e,
                                                  const GlmWindow& win, bool second, const double* __restrict__ coef,
                                                  int64_t batch, int lane) {
#pragma unroll
    for (int u = 0; u < kGlmU; u++) {
        const int64_t i = b + u * 64 + lane;
        p[u] = 0.0;
        if (i < e) {
            const int64_t j = glm_batch_pos(win, csc_row[i], second);
            if ((uint64_t)j < (uint64_t)batch) p[u] = csc_val[i] * coef[j];
        }
    }
}
// One range of a long column by the whole wave: the products of kGlmU * 64 entries go to the wave's
// LDS slots and are added from there in order, while the loads, gathers and products of the next
// kGlmU * 64 entries are in flight.  s and e are wave-uniform.  A wave's LDS accesses execute in
// program order, and the wavefront-scope fences keep the compiler to it; no other wave sees the slots.
__device__ __forceinline__ double glm_wave_range_sum(double acc, const int32_t* __restrict__ csc_row,
                                                     const double* __restrict__ csc_val, int64_t s, int64_t e,
                                                     const GlmWindow& win, bool second,
                                                     const double* __restrict__ coef, int64_t batch, int lane,
                                                     double* slots) {
    if (s >= e) return acc;
    constexpr int64_t kStep = (int64_t)kGlmU * 64;
    double nxt[kGlmU];
    glm_load_products(nxt, csc_row, csc_val, s, e, win, second, coef, batch, lane);
    for (int64_t b = s; b < e; b += kStep) {
#pragma unroll
        for (int u = 0; u < kGlmU; u++) slots[u * 64 + lane] = nxt[u];
        if (b + kStep < e) glm_load_products(nxt, csc_row, csc_val, b + kStep, e, win, second, coef, batch, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < kGlmU; u++) {
            const int64_t rem = e - (b + u * 64);
            if (rem > 0) acc = ordered_add_lds(acc, slots + u * 64, (int)std::min<int64_t>(64, rem));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_glm_plus_by(skml_glm_data d, GlmWindow win, int64_t batch,
                                                     const double* __restrict__ coef, double* __restrict__ g,
                                                     unsigned long long* count) {
    __shared__ unsigned long long s_cnt;
    __shared__ double s_prod[4][kGlmU * 64];  // the wave form's products, a wave's own slots
    const int lane = threadIdx.x & 63;
    double* slots = s_prod[threadIdx.x >> 6];
    const int64_t gstep = (int64_t)gridDim.x * 256;
    LiveCount lc;
    // the trip count is the wave's: the ballots and the wave form need every lane
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); base < d.dim; base += gstep) {
        const int64_t k = base + lane;
        const bool on = k < d.dim;
        double acc = 0.0;
        GlmColRanges r{0, 0, 0, 0};
        bool big = false;
        if (on) {
            const int64_t cs = clamp_ptr(d.col_ptr[k], d.nnz), ce = clamp_ptr(d.col_ptr[k + 1], d.nnz);
            if (ce > cs) {
                r = glm_col_ranges(d.csc_row, cs, ce, win);
                if (r.count() <= kGlmLaneMax) acc = glm_col_sum(d.csc_row, d.csc_val, r, win, coef, batch);
                else big = true;
            }
        }
        for (unsigned long long m = __ballot(big); m; m &= m - 1) {
            const int src = __ffsll((long long)m) - 1;
            const int64_t s0 = uniform_i64(r.s0, src), e0 = uniform_i64(r.e0, src);
            const int64_t s1 = uniform_i64(r.s1, src), e1 = uniform_i64(r.e1, src);
            double a = glm_wave_range_sum(0.0, d.csc_row, d.csc_val, s0, e0, win, false, coef, batch, lane, slots);
            a = glm_wave_range_sum(a, d.csc_row, d.csc_val, s1, e1, win, true, coef, batch, lane, slots);
            if (lane == src) acc = a;
        }
        if (on) g[k] = acc;
        lc.add(on && fabs(acc) > 1e-8);  // DenseDoubleGradient.countNNZ
    }
    lc.finish(&s_cnt, count);
}

// Java's Math.max / Math.min: a NaN wins, and -0.0 < +0.0.
__device__ __forceinline__ double java_max(double a, double b) {
    if (a != a) return a;
    if (a == 0.0 && b == 0.0 && signbit(a)) return b;
    return a >= b ? a : b;
}
__device__ __forceinline__ double java_min(double a, double b) {
    if (a != a) return a;
    if (a == 0.0 && b == 0.0 && signbit(b)) return b;
    return a <= b ? a : b;
}

template <typename W>
__global__ __launch_bounds__(256) void k_glm_finish(const int32_t* __restrict__ keys, double* __restrict__ vals,
                                                    int64_t n, int64_t dim, double times, int reg, double theta,
                                                    const W* __restrict__ w) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double v = vals[i] * times;  // timesBy
        if (reg == SKML_REG_L1) {    // l1Reg(grad, 0, theta)
            const double alpha = 0.0;
            if (v >= 0 && v <= theta) v = java_max(v - alpha, 0.0);
            else if (v < 0 && v >= -theta) v = java_min(v - alpha, 0.0);
        } else if (reg == SKML_REG_L2) {  // l2Reg: v(i) += w(k(i)) * lambda
            const int64_t k = keys ? (int64_t)keys[i] : i;
            if ((uint64_t)k < (uint64_t)dim) {
                const double t = (double)w[k] * theta;
                v += t;
            }
        }
        vals[i] = v;
    }
}

// ---- launchers ----
static unsigned glm_grid(int64_t items, int64_t per_block, int64_t cap) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, cap));
}

int glm_lanes_per_row(int64_t nnz, int64_t rows) {
    const int64_t mean = rows > 0 ? nnz / rows : 0;
    return mean <= 4 ? 1 : (mean <= 32 ? 8 : 64);
}

template <typename W, int LOSS, int LPR>
static void launch_predict_l(hipStream_t st, const skml_glm_data& d, const GlmWindow& win, int64_t batch, const void* w,
                             double* pre, double* coef, double* loss) {
    hipLaunchKernelGGL((k_glm_predict<W, LOSS, LPR>), dim3(glm_grid(batch, 256 / LPR, 65536)), dim3(256), 0, st, d, win,
                       batch, static_cast<const W*>(w), pre, coef, loss);
}
template <typename W, int LOSS>
static void launch_predict_w(hipStream_t st, const skml_glm_data& d, const GlmWindow& win, int64_t batch, const void* w,
                             int lanes, double* pre, double* coef, double* loss) {
    if (lanes == 1) launch_predict_l<W, LOSS, 1>(st, d, win, batch, w, pre, coef, loss);
    else if (lanes == 8) launch_predict_l<W, LOSS, 8>(st, d, win, batch, w, pre, coef, loss);
    else launch_predict_l<W, LOSS, 64>(st, d, win, batch, w, pre, coef, loss);
}
template <typename W>
static hipError_t launch_predict(hipStream_t st, const skml_glm_data& d, const GlmWindow& win, int64_t batch,
                                 int loss_kind, const void* w, int lanes, double* pre, double* coef, double* loss) {
    switch (loss_kind) {
        case SKML_LOSS_L1_LOG:
        case SKML_LOSS_L2_LOG: launch_predict_w<W, kGlmLog>(st, d, win, batch, w, lanes, pre, coef, loss); break;
        case SKML_LOSS_L2_HINGE: launch_predict_w<W, kGlmHinge>(st, d, win, batch, w, lanes, pre, coef, loss); break;
        case SKML_LOSS_L2_SQUARE: launch_predict_w<W, kGlmSquare>(st, d, win, batch, w, lanes, pre, coef, loss); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_glm_predict(hipStream_t st, const skml_glm_data& d, int64_t row0, int64_t batch, int loss_kind,
                              const void* w, int wide, int lanes, double* pre, double* coef, double* loss) {
    if (batch < 1 || batch > d.rows || row0 < 0 || row0 >= d.rows || (lanes != 1 && lanes != 8 && lanes != 64))
        return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    return wide ? launch_predict<double>(st, d, win, batch, loss_kind, w, lanes, pre, coef, loss)
                : launch_predict<float>(st, d, win, batch, loss_kind, w, lanes, pre, coef, loss);
}

template <typename W, int LOSS>
static void launch_valid_w(hipStream_t st, const skml_glm_data& d, const void* w, int lanes, double* pre, double* loss,
                           unsigned long long* cnt) {
    const W* wp = static_cast<const W*>(w);
    if (lanes == 1)
        hipLaunchKernelGGL((k_glm_valid<W, LOSS, 1>), dim3(glm_grid(d.rows, 256, 65536)), dim3(256), 0, st, d, wp, pre, loss, cnt);
    else if (lanes == 8)
        hipLaunchKernelGGL((k_glm_valid<W, LOSS, 8>), dim3(glm_grid(d.rows, 32, 65536)), dim3(256), 0, st, d, wp, pre, loss, cnt);
    else
        hipLaunchKernelGGL((k_glm_valid<W, LOSS, 64>), dim3(glm_grid(d.rows, 4, 65536)), dim3(256), 0, st, d, wp, pre, loss, cnt);
}
template <typename W>
static hipError_t launch_valid(hipStream_t st, const skml_glm_data& d, int loss_kind, const void* w, int lanes, double* pre,
                               double* loss, unsigned long long* cnt) {
    switch (loss_kind) {
        case SKML_LOSS_L1_LOG:
        case SKML_LOSS_L2_LOG: launch_valid_w<W, kGlmLog>(st, d, w, lanes, pre, loss, cnt); break;
        case SKML_LOSS_L2_HINGE: launch_valid_w<W, kGlmHinge>(st, d, w, lanes, pre, loss, cnt); break;
        case SKML_LOSS_L2_SQUARE: launch_valid_w<W, kGlmSquare>(st, d, w, lanes, pre, loss, cnt); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_glm_valid(hipStream_t st, const skml_glm_data& d, int loss_kind, const void* w, int wide, int lanes,
                            double* pre, double* loss, unsigned long long* cnt) {
    if (d.rows < 1 || !loss || !cnt || (lanes != 1 && lanes != 8 && lanes != 64)) return hipErrorInvalidValue;
    return wide ? launch_valid<double>(st, d, loss_kind, w, lanes, pre, loss, cnt)
                : launch_valid<float>(st, d, loss_kind, w, lanes, pre, loss, cnt);
}

hipError_t launch_glm_seq_sum(hipStream_t st, const double* x, int64_t n, double* out) {
    hipLaunchKernelGGL(k_glm_seq_sum, dim3(1), dim3(64), 0, st, x, n, out);
    return hipGetLastError();
}

hipError_t launch_glm_loss_sum(hipStream_t st, const double* loss, int64_t batch, double* obj) {
    hipLaunchKernelGGL(k_glm_loss_sum, dim3(1), dim3(1024), 0, st, loss, batch, obj);
    return hipGetLastError();
}

hipError_t launch_glm_plus_by(hipStream_t st, const skml_glm_data& d, int64_t row0, int64_t batch, const double* coef,
                              double* g, unsigned long long* count) {
    if (batch < 1 || batch > d.rows || row0 < 0 || row0 >= d.rows || d.dim < 1) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    hipLaunchKernelGGL(k_glm_plus_by, dim3(glm_grid(d.dim, 256, 16384)), dim3(256), 0, st, d, win, batch, coef, g, count);
    return hipGetLastError();
}

hipError_t launch_glm_finish(hipStream_t st, const int32_t* keys, double* vals, int64_t n, int64_t dim, double times,
                             int reg_kind, double reg_param, const void* w, int wide) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = glm_grid(n, 256, 16384);
    if (wide)
        hipLaunchKernelGGL(k_glm_finish<double>, dim3(grid), dim3(256), 0, st, keys, vals, n, dim, times, reg_kind, reg_param,
                           static_cast<const double*>(w));
    else
        hipLaunchKernelGGL(k_glm_finish<float>, dim3(grid), dim3(256), 0, st, keys, vals, n, dim, times, reg_kind, reg_param,
                           static_cast<const float*>(w));
    return hipGetLastError();
}

}  // namespace skml
