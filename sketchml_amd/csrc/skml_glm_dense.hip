// skml_glm_dense.hip -- the mini-batch gradient and the validation pass over dense instances
// (Parser.parseCSV -> Vectors.dense; Maths.dot(DenseVector, DenseVector), ml/util/Maths.scala:44-55;
// DenseDoubleGradient.plusBy(DenseVector, x), DenseDoubleGradient.scala:44-49).  x is rows * dim doubles,
// row-major.  The contract is the sparse path's (include/skml.h): every sum is one chain of rounded
// adds from +0.0 in index order, every product rounded before it is added, so the only parallelism is
// across chains and no matrix instruction fits (v_mfma_f64_* accumulates in an order of its own).
//   k_glm_dense_predict<W, LOSS>  a lane owns a batch position and runs its row's chain alone; the
//                                 wave stages 64 rows x kDenseC columns through its own two LDS slabs:
//                                 loaded along the rows (coalesced), stored transposed and padded,
//                                 read back lane = row.  The next tile's loads are in flight while
//                                 the chain over the current one runs.  Then loss.loss / -1.0 * loss.grad
//   k_glm_dense_valid<W, LOSS>    the same dot over every row, loss.loss, the confusion counts
//   k_glm_dense_plus_by           a lane owns a column; the wave streams the window's rows in batch
//                                 order, kDenseU rows of loads in flight ahead of the dependent add,
//                                 one wave-uniform coef_j per row; toAuto's live count on the way
// The tile arithmetic is skml_glm_dense.hpp's, shared with tests/glm_dense_check.cpp; the window is
// skml_glm.hpp's; the losses and the counts are skml_glm_device.hpp's.
#include <algorithm>

#include "skml_device.hpp"
#include "skml_glm_dense.hpp"
#include "skml_glm_device.hpp"
#include "skml_opt.hpp"

namespace skml {

// The lane's kDenseLoads values of the tile at column c0; +0.0 where the tile has no row or column.
// off[i]: the first element of the row of load i, -1 without one.  A lane without an element reads
// x[0] and drops it, so the loads of a tile issue back to back with no branch between them.
__device__ __forceinline__ void dense_tile_load(double (&v)[kDenseLoads], const double* __restrict__ x,
                                                const int64_t (&off)[kDenseLoads], int64_t c0, int64_t dim, int col) {
    const bool in = c0 + col < dim;
#pragma unroll
    for (int i = 0; i < kDenseLoads; i++) {
        const bool has = in && off[i] >= 0;
        const double e = x[has ? off[i] + c0 + col : 0];
        v[i] = has ? e : 0.0;
    }
}

// Maths.dot(w, x_row) for the 64 batch positions from jb on, lane = position: +0.0, then
// (double)w[c] * x[row][c] rounded and added for c = 0 .. dim - 1.  slabs: the wave's own kDenseWaveLds
// bytes.  A wave's LDS accesses execute in program order and no other wave sees the slabs, so a
// wavefront-scope fence (which keeps the compiler to that order) is all that separates a slab's
// stores from its reads; a slab is stored again two fences after its last read.  jb is wave-uniform.
template <typename W>
__device__ __forceinline__ double dense_row_dots(const double* __restrict__ x, int64_t dim, const GlmWindow& win,
                                                 int64_t batch, int64_t jb, const W* __restrict__ w, double* slabs) {
    const int lane = threadIdx.x & 63;
    const int col = dense_load_col(lane);
    int64_t off[kDenseLoads];
#pragma unroll
    for (int i = 0; i < kDenseLoads; i++) {
        const int64_t j = jb + dense_load_row(i, lane);
        off[i] = j < batch ? glm_row_of(win, j) * dim : -1;
    }
    double nxt[kDenseLoads];
    dense_tile_load(nxt, x, off, 0, dim, col);
    double acc = 0.0;
    int t = 0;
    for (int64_t c0 = 0; c0 < dim; c0 += kDenseC, t ^= 1) {
        double* slab = slabs + t * kDenseSlab;
#pragma unroll
        for (int i = 0; i < kDenseLoads; i++) slab[dense_slab_index(col, dense_load_row(i, lane))] = nxt[i];
        if (c0 + kDenseC < dim) dense_tile_load(nxt, x, off, c0 + kDenseC, dim, col);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int cn = dense_tile_cols(dim, c0);
        if (cn == kDenseC) {
#pragma unroll
            for (int c = 0; c < kDenseC; c++) {
                const double p = (double)w[c0 + c] * slab[dense_slab_index(c, lane)];
                acc += p;
            }
        } else {
            for (int c = 0; c < cn; c++) {
                const double p = (double)w[c0 + c] * slab[dense_slab_index(c, lane)];
                acc += p;
            }
        }
    }
    return acc;
}

// blockDim.x = 64 * waves per workgroup; dynamic LDS: kDenseWaveLds bytes per wave.
template <typename W, int LOSS>
__global__ __launch_bounds__(64 * kDenseMaxWaves) void k_glm_dense_predict(
    const double* __restrict__ x, const double* __restrict__ label, int64_t dim, GlmWindow win, int64_t batch,
    const W* __restrict__ w, double* __restrict__ pre, double* __restrict__ coef, double* __restrict__ loss) {
    extern __shared__ double s_slabs[];
    const int wave = threadIdx.x >> 6;
    const int64_t jb = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * 64;
    if (jb >= batch) return;  // the whole wave: nothing below crosses waves
    const double acc = dense_row_dots<W>(x, dim, win, batch, jb, w, s_slabs + wave * 2 * kDenseSlab);
    const int64_t j = jb + (threadIdx.x & 63);
    if (j < batch) {
        double l, g;
        glm_loss<LOSS>(acc, label[glm_row_of(win, j)], l, g);
        if (pre) pre[j] = acc;
        coef[j] = -1.0 * g;
        if (loss) loss[j] = l;
    }
}

template <typename W, int LOSS>
__global__ __launch_bounds__(64 * kDenseMaxWaves) void k_glm_dense_valid(
    const double* __restrict__ x, const double* __restrict__ label, int64_t rows, int64_t dim, const W* __restrict__ w,
    double* __restrict__ pre, double* __restrict__ loss, unsigned long long* __restrict__ cnt) {
    extern __shared__ double s_slabs[];
    __shared__ unsigned long long s_cnt[kValidCounters];
    const int wave = threadIdx.x >> 6;
    const int64_t jb = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * 64;
    const GlmWindow win{0, rows, 0};
    ValidCount vc;
    int cls = kValidNone;
    bool nan = false;
    if (jb < rows) {  // wave-uniform; every wave reaches the counts below
        const double acc = dense_row_dots<W>(x, dim, win, rows, jb, w, s_slabs + wave * 2 * kDenseSlab);
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

// g[k] = +0.0, then x[row_j][k] * coef[j] rounded and added for j = 0 .. batch - 1; count += #{|g[k]| > 1e-8}.
// The row's first element and coef[j] are wave-uniform (scalar loads, one address register per row);
// a lane's kDenseV columns are 64 apart, so every load of the wave reads 512 contiguous bytes.
__global__ __launch_bounds__(256) void k_glm_dense_plus_by(const double* __restrict__ x, int64_t dim, GlmWindow win,
                                                           int64_t batch, const double* __restrict__ coef,
                                                           double* __restrict__ g, unsigned long long* count) {
    __shared__ unsigned long long s_cnt;
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * kDenseWaveCols;
    bool on[kDenseV];
    int64_t k[kDenseV], kl[kDenseV];  // kl: the column the lane loads, column 0 (dropped) past dim
    double acc[kDenseV];
#pragma unroll
    for (int v = 0; v < kDenseV; v++) {
        k[v] = dense_col_of(base, v, lane);
        on[v] = k[v] < dim;
        kl[v] = on[v] ? k[v] : 0;
        acc[v] = 0.0;
    }
    if (base < dim) {  // wave-uniform
        int64_t j = 0;
        for (; j + kDenseU <= batch; j += kDenseU) {
            double xv[kDenseU][kDenseV];
#pragma unroll
            for (int u = 0; u < kDenseU; u++) {
                const double* row = x + glm_row_of(win, j + u) * dim;
#pragma unroll
                for (int v = 0; v < kDenseV; v++) xv[u][v] = row[kl[v]];
            }
#pragma unroll
            for (int u = 0; u < kDenseU; u++) {
                const double c = coef[j + u];
#pragma unroll
                for (int v = 0; v < kDenseV; v++) {
                    const double p = xv[u][v] * c;
                    acc[v] += p;
                }
            }
        }
        for (; j < batch; j++) {  // the last batch % kDenseU rows: an exact trip count
            const double* row = x + glm_row_of(win, j) * dim;
            const double c = coef[j];
#pragma unroll
            for (int v = 0; v < kDenseV; v++) {
                const double p = row[kl[v]] * c;
                acc[v] += p;
            }
        }
    }
    LiveCount lc;
#pragma unroll
    for (int v = 0; v < kDenseV; v++) {
        if (on[v]) g[k[v]] = acc[v];
        lc.add(on[v] && fabs(acc[v]) > 1e-8);  // DenseDoubleGradient.countNNZ
    }
    lc.finish(&s_cnt, count);
}

// ---- launchers ----
template <typename W>
static hipError_t launch_dense_predict_w(hipStream_t st, const skml_glm_dense_data& d, const GlmWindow& win, int64_t batch,
                                         int loss_kind, const W* w, double* pre, double* coef, double* loss) {
    const int64_t waves = dense_row_waves(batch);
    const int wpg = dense_waves_per_group(waves);
    const dim3 grid((unsigned)((waves + wpg - 1) / wpg)), block(64 * wpg);
    const size_t lds = (size_t)wpg * kDenseWaveLds;
    switch (loss_kind) {
        case SKML_LOSS_L1_LOG:
        case SKML_LOSS_L2_LOG:
            hipLaunchKernelGGL((k_glm_dense_predict<W, kGlmLog>), grid, block, lds, st, d.x, d.label, d.dim, win, batch, w, pre, coef, loss);
            break;
        case SKML_LOSS_L2_HINGE:
            hipLaunchKernelGGL((k_glm_dense_predict<W, kGlmHinge>), grid, block, lds, st, d.x, d.label, d.dim, win, batch, w, pre, coef, loss);
            break;
        case SKML_LOSS_L2_SQUARE:
            hipLaunchKernelGGL((k_glm_dense_predict<W, kGlmSquare>), grid, block, lds, st, d.x, d.label, d.dim, win, batch, w, pre, coef, loss);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_glm_dense_predict(hipStream_t st, const skml_glm_dense_data& d, int64_t row0, int64_t batch, int loss_kind,
                                    const void* w, int wide, double* pre, double* coef, double* loss) {
    if (batch < 1 || batch > d.rows || row0 < 0 || row0 >= d.rows || d.dim < 1 || !coef) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    return wide ? launch_dense_predict_w(st, d, win, batch, loss_kind, static_cast<const double*>(w), pre, coef, loss)
                : launch_dense_predict_w(st, d, win, batch, loss_kind, static_cast<const float*>(w), pre, coef, loss);
}

template <typename W>
static hipError_t launch_dense_valid_w(hipStream_t st, const skml_glm_dense_data& d, int loss_kind, const W* w, double* pre,
                                       double* loss, unsigned long long* cnt) {
    const int64_t waves = dense_row_waves(d.rows);
    const int wpg = dense_waves_per_group(waves);
    const dim3 grid((unsigned)((waves + wpg - 1) / wpg)), block(64 * wpg);
    const size_t lds = (size_t)wpg * kDenseWaveLds;
    switch (loss_kind) {
        case SKML_LOSS_L1_LOG:
        case SKML_LOSS_L2_LOG:
            hipLaunchKernelGGL((k_glm_dense_valid<W, kGlmLog>), grid, block, lds, st, d.x, d.label, d.rows, d.dim, w, pre, loss, cnt);
            break;
        case SKML_LOSS_L2_HINGE:
            hipLaunchKernelGGL((k_glm_dense_valid<W, kGlmHinge>), grid, block, lds, st, d.x, d.label, d.rows, d.dim, w, pre, loss, cnt);
            break;
        case SKML_LOSS_L2_SQUARE:
            hipLaunchKernelGGL((k_glm_dense_valid<W, kGlmSquare>), grid, block, lds, st, d.x, d.label, d.rows, d.dim, w, pre, loss, cnt);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_glm_dense_valid(hipStream_t st, const skml_glm_dense_data& d, int loss_kind, const void* w, int wide,
                                  double* pre, double* loss, unsigned long long* cnt) {
    if (d.rows < 1 || d.dim < 1 || !loss || !cnt) return hipErrorInvalidValue;
    return wide ? launch_dense_valid_w(st, d, loss_kind, static_cast<const double*>(w), pre, loss, cnt)
                : launch_dense_valid_w(st, d, loss_kind, static_cast<const float*>(w), pre, loss, cnt);
}

hipError_t launch_glm_dense_plus_by(hipStream_t st, const skml_glm_dense_data& d, int64_t row0, int64_t batch,
                                    const double* coef, double* g, unsigned long long* count) {
    if (batch < 1 || batch > d.rows || row0 < 0 || row0 >= d.rows || d.dim < 1) return hipErrorInvalidValue;
    const GlmWindow win = glm_window(d.rows, row0, batch);
    const int64_t waves = dense_col_waves(d.dim);
    const int threads = dense_col_threads(waves);
    const int64_t per = threads / 64;
    hipLaunchKernelGGL(k_glm_dense_plus_by, dim3((unsigned)((waves + per - 1) / per)), dim3(threads), 0, st, d.x, d.dim, win,
                       batch, coef, g, count);
    return hipGetLastError();
}

}  // namespace skml
