// skml_glm_api.cpp -- host side of the mini-batch gradient of the C ABI (include/skml.h;
// ml/objective/GradientDescent.scala:23-87).  Every entry family is its argument checks (skml_glm_args.hpp), then
// gradient_run with the three steps that differ between the families: predict, the loss sum and the column sum.
// gradient_run owns the context buffer that stands in for the arrays the caller does not keep, and the one
// read-back of toAuto's counts and objLoss.
#include "skml_glm_dense.hpp"
#include "skml_glm_dense_blocked.hpp"
#include "skml_glm_segmented.hpp"
#include "skml_host.hpp"

using namespace skml;

namespace {

// The head of the workspace, read back as one block: the live counters of up to kMulMaxModels models, then their
// objLoss.  The stand-ins for coef and loss (K x batch doubles each) follow it.
constexpr size_t kGlmHead = 256;
static_assert(kGlmHead >= 16 * kMulMaxModels, "K live counters and K objLoss ahead of the stand-in arrays");

// What every family runs once its arguments are checked, for K = models (1 for all but the K-model entries):
// predict(coef, loss) and loss_sum(loss, obj) under one timing id, col_sum(coef, cnt) under the other, then the one
// synchronisation.  A step returns the library's status: a HIP failure through HIP_TRY, a failed reserve as it is.
template <typename Predict, typename LossSum, typename ColSum>
int gradient_run(skml_ctx* c, int models, int64_t batch, const GlmOut& o, Predict predict, LossSum loss_sum, ColSum col_sum) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t bb = (size_t)models * (size_t)batch * 8, need = kGlmHead + 2 * bb;
    if (const int st = reserve(c, c->glm_ws, need, need + need / 4, "the mini-batch gradient's workspace")) return st;
    char* base = static_cast<char*>(c->glm_ws.p);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(base);
    double* obj = reinterpret_cast<double*>(base + 8 * kMulMaxModels);
    double* coef = o.coef ? o.coef : reinterpret_cast<double*>(base + kGlmHead);
    double* loss = o.loss ? o.loss : reinterpret_cast<double*>(base + kGlmHead + bb);
    unsigned long long* pin = static_cast<unsigned long long*>(ctx_pinned(c, kGlmHead));
    if (!pin) return fail(SKML_E_OOM, "pinned staging of the live counts and objLoss");

    HIP_TRY(hipMemsetAsync(base, 0, kGlmHead, c->stream));
    {
        KernelTimer kt(c, SKML_K_GLM_PREDICT);
        if (const int st = predict(coef, loss)) return st;
        if (const int st = loss_sum(loss, obj)) return st;
    }
    {
        KernelTimer kt(c, SKML_K_GLM_PLUS_BY);
        if (const int st = col_sum(coef, cnt)) return st;
    }
    HIP_TRY(hipMemcpyAsync(pin, base, kGlmHead, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    static_assert(sizeof(double) == sizeof(pin[0]), "objLoss travels as 8 bytes");
    for (int m = 0; m < models; m++) {
        o.nnz[m] = (int64_t)pin[m];
        __builtin_memcpy(&o.obj_loss[m], &pin[kMulMaxModels + m], 8);
    }
    return SKML_OK;
}

// The loss sum of the single-model families.
auto loss_sum_one(skml_ctx* c, int64_t batch) {
    return [=](const double* loss, double* obj) -> int {
        HIP_TRY(launch_glm_loss_sum(c->stream, loss, batch, obj));
        return SKML_OK;
    };
}

// Sparse instances.  kSegmented: the column sum of skml_glm_segmented.hip in place of k_glm_plus_by; its work list
// and partial sums live in the context's staging, reserved inside the step, after every check.
template <bool kSegmented>
int gradient_x(skml_ctx* c, const skml_glm_data* d, int64_t row0, int64_t batch, int32_t loss_kind, const void* w, int wide,
               const GlmOut& o) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    if (const int st = sparse_check(d)) return st;
    if (const int st = window_check(d->rows, row0, batch)) return st;
    if (const int st = loss_check(loss_kind)) return st;
    const size_t nz = (size_t)d->nnz, bb = (size_t)batch * 8;
    const Range in[] = {{d->row_ptr, ((size_t)d->rows + 1) * 8, "row_ptr"}, {d->col, nz * 4, "col"}, {d->val, nz * 8, "val"},
                        {d->label, (size_t)d->rows * 8, "label"}, {d->col_ptr, ((size_t)d->dim + 1) * 8, "col_ptr"},
                        {d->csc_row, nz * 4, "csc_row"}, {d->csc_val, nz * 8, "csc_val"},
                        {w, (size_t)d->dim * (wide ? 8 : 4), "w"}};
    const Range out[] = {{o.pre, bb, "pre_out"}, {o.coef, bb, "coef_out"}, {o.loss, bb, "loss_out"}};
    const Range grad{o.grad, (size_t)d->dim * 8, "grad_out"};
    if (!d->row_ptr || !d->label || !d->col_ptr || !w || !o.grad) return fail(SKML_E_ARG, "row_ptr, label, col_ptr, w or grad_out is NULL");
    if (nz && (!d->col || !d->val || !d->csc_row || !d->csc_val)) return fail(SKML_E_ARG, "col, val, csc_row or csc_val is NULL");
    if (!o.nnz || !o.obj_loss) return fail(SKML_E_ARG, "nnz_out or obj_loss_out is NULL");
    if (const int st = ranges_check(in, 8, out, 3, &grad)) return st;

    return gradient_run(
        c, 1, batch, o,
        [&](double* coef, double* loss) -> int {
            HIP_TRY(launch_glm_predict(c->stream, *d, row0, batch, loss_kind, w, wide, glm_lanes_per_row(d->nnz, d->rows), o.pre, coef, loss));
            return SKML_OK;
        },
        loss_sum_one(c, batch),
        [&](const double* coef, unsigned long long* cnt) -> int {
            if (!kSegmented) {
                HIP_TRY(launch_glm_plus_by(c->stream, *d, row0, batch, coef, o.grad, cnt));
                return SKML_OK;
            }
            const size_t need = (size_t)seg_stage_bytes(d->dim, d->nnz);
            if (const int st = reserve(c, c->stage, need, need + need / 4, "the segmented gradient's work list")) return st;
            HIP_TRY(launch_glm_segmented_plus_by(c->stream, *d, row0, batch, coef, c->stage.p, o.grad, cnt));
            return SKML_OK;
        });
}

// The checks of every dense family, over either dense struct: the context, the struct (into *v), then the rest.
template <typename Data>
int dense_args(skml_ctx* c, const Data* d, int64_t row0, int64_t batch, int32_t loss_kind, int32_t models, const void* w, int wide,
               const double* labels, const GlmOut& o, DenseView* v) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    if (const int st = dense_view(d, v)) return st;
    return dense_gradient_check(v->bx.rows, v->bx.dim, v->bx.x, v->bytes, v->bx.label, row0, batch, loss_kind, models, w, wide, labels, o);
}

// Dense instances in the reference's sequential order: the launchers of skml_glm_dense.hip for a double x, of
// skml_glm_dense_lowp.hip for an x stored as fp32, bf16 or fp16.
template <typename Data, auto LaunchPredict, auto LaunchPlusBy>
int gradient_dense_x(skml_ctx* c, const Data* d, int64_t row0, int64_t batch, int32_t loss_kind, const void* w, int wide,
                     const GlmOut& o) {
    DenseView v;
    if (const int st = dense_args(c, d, row0, batch, loss_kind, 1, w, wide, nullptr, o, &v)) return st;
    return gradient_run(
        c, 1, batch, o,
        [&](double* coef, double* loss) -> int {
            HIP_TRY(LaunchPredict(c->stream, *d, row0, batch, loss_kind, w, wide, o.pre, coef, loss));
            return SKML_OK;
        },
        loss_sum_one(c, batch),
        [&](const double* coef, unsigned long long* cnt) -> int {
            HIP_TRY(LaunchPlusBy(c->stream, *d, row0, batch, coef, o.grad, cnt));
            return SKML_OK;
        });
}

// Dense instances in the blocked summation order (skml_glm_dense_blocked.hip).  The partial sums of the column sum
// live in the context's staging buffer, reserved inside the step: every use of that buffer is ordered on the
// context's stream, and gradient_run's own workspace is not moved under it.
template <typename Data>
int gradient_dense_blocked_x(skml_ctx* c, const Data* d, int64_t row0, int64_t batch, int32_t loss_kind, const void* w, int wide,
                             const GlmOut& o) {
    DenseView v;
    if (const int st = dense_args(c, d, row0, batch, loss_kind, 1, w, wide, nullptr, o, &v)) return st;
    return gradient_run(
        c, 1, batch, o,
        [&](double* coef, double* loss) -> int {
            HIP_TRY(launch_glm_dense_blocked_predict(c->stream, v.bx, row0, batch, loss_kind, w, wide, o.pre, coef, loss));
            return SKML_OK;
        },
        loss_sum_one(c, batch),
        [&](const double* coef, unsigned long long* cnt) -> int {
            BlkPlan plan;
            if (!blk_plan(v.x_bytes, batch, v.bx.dim, &plan)) return fail(SKML_E_ARG, "no plan for batch=%lld, dim=%lld", (long long)batch, (long long)v.bx.dim);
            const size_t need = (size_t)plan.ws_bytes;
            if (need)
                if (const int st = reserve(c, c->stage, need, need + need / 4, "the blocked gradient's partial sums")) return st;
            HIP_TRY(launch_glm_dense_blocked_plus_by(c->stream, v.bx, row0, batch, coef, need ? static_cast<double*>(c->stage.p) : nullptr, o.grad, cnt));
            return SKML_OK;
        });
}

// Dense instances, K <= 16 models in one pass over x (skml_glm_dense_multi.hip): K-fold arrays, K counters and K
// objLoss; the partial sums live in the staging buffer as the blocked order's do.
template <typename Data>
int gradient_dense_multi_x(skml_ctx* c, const Data* d, int64_t row0, int64_t batch, int32_t loss_kind, int32_t models, const void* w,
                           int wide, const double* labels, const GlmOut& o) {
    DenseView v;
    if (const int st = dense_args(c, d, row0, batch, loss_kind, models, w, wide, labels, o, &v)) return st;
    MulPlan plan;
    if (!mul_plan(v.x_bytes, models, batch, v.bx.dim, &plan))
        return fail(SKML_E_ARG, "no plan for %d models, batch=%lld, dim=%lld", models, (long long)batch, (long long)v.bx.dim);
    return gradient_run(
        c, models, batch, o,
        [&](double* coef, double* loss) -> int {
            HIP_TRY(launch_glm_dense_multi_predict(c->stream, v.bx, row0, batch, loss_kind, w, wide, models, labels, o.pre, coef, loss));
            return SKML_OK;
        },
        [&](const double* loss, double* obj) -> int {
            HIP_TRY(launch_glm_dense_multi_loss_sum(c->stream, loss, batch, models, obj));
            return SKML_OK;
        },
        [&](const double* coef, unsigned long long* cnt) -> int {
            const size_t need = (size_t)plan.ws_bytes;
            if (need)
                if (const int st = reserve(c, c->stage, need, need + need / 4, "the multi-model gradient's partial sums")) return st;
            HIP_TRY(launch_glm_dense_multi_plus_by(c->stream, v.bx, row0, batch, coef, models, need ? static_cast<double*>(c->stage.p) : nullptr, o.grad, cnt));
            return SKML_OK;
        });
}

int finish_x(skml_ctx* c, const int32_t* keys, bool kv, double* vals, int64_t n, int64_t dim, double times, int32_t reg_kind,
             double reg_param, const void* w, int32_t w_fp32) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (dim < 1 || dim > kJavaIntMax) return fail(SKML_E_ARG, "dim=%lld outside [1, 2^31 - 1]", (long long)dim);
    if (n < 0 || n > dim) return fail(SKML_E_ARG, "nnz=%lld outside [0, dim]", (long long)n);
    if (reg_kind != SKML_REG_NONE && reg_kind != SKML_REG_L1 && reg_kind != SKML_REG_L2)
        return fail(SKML_E_ARG, "unknown regulariser %d", reg_kind);
    if (n > 0 && (!vals || (kv && !keys))) return fail(SKML_E_ARG, "the values or the keys are NULL");
    if (!aligned8(vals) || ((uintptr_t)keys) % 4) return fail(SKML_E_ARG, "the values must be 8-byte and the keys 4-byte aligned");
    if (reg_kind == SKML_REG_L2 && !w) return fail(SKML_E_ARG, "SKML_REG_L2 needs w");
    if (w && ((uintptr_t)w) % (w_fp32 ? 4 : 8)) return fail(SKML_E_ARG, "w is misaligned");
    const Range rv{vals, (size_t)n * 8, "the values"}, rk{keys, (size_t)n * 4, "the keys"},
        rw{w, (size_t)dim * (w_fp32 ? 4 : 8), "w"};
    if (overlap(rv, rw) || overlap(rv, rk)) return fail(SKML_E_ARG, "the values overlap w or the keys");
    HIP_TRY(hipSetDevice(c->device));
    KernelTimer kt(c, SKML_K_GLM_FINISH);
    HIP_TRY(launch_glm_finish(c->stream, kv ? keys : nullptr, vals, n, dim, times, reg_kind, reg_param, w, !w_fp32));
    return SKML_OK;
}

}  // namespace

extern "C" {

// The gradient entries only forward: `...` is the family's function above, w_t the weight's type.
#define SKML_GRADIENT_ENTRY(name, data_t, w_t, ...)                                                                                   \
    int name(skml_ctx* c, const data_t* data, int64_t row0, int64_t batch, int32_t loss_kind, const w_t* w, double* pre_out,         \
             double* coef_out, double* loss_out, double* grad_out, int64_t* nnz_out, double* obj_loss_out) {                         \
        return __VA_ARGS__(c, data, row0, batch, loss_kind, w, sizeof(w_t) == 8,                                                      \
                           GlmOut{pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out});                                    \
    }
#define SKML_GRADIENT_MULTI_ENTRY(name, data_t, w_t)                                                                                  \
    int name(skml_ctx* c, const data_t* data, int64_t row0, int64_t batch, int32_t loss_kind, int32_t models, const w_t* w,          \
             const double* labels, double* pre_out, double* coef_out, double* loss_out, double* grad_out, int64_t* nnz_out,          \
             double* obj_loss_out) {                                                                                                 \
        return gradient_dense_multi_x(c, data, row0, batch, loss_kind, models, w, sizeof(w_t) == 8, labels,                          \
                                      GlmOut{pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out});                         \
    }
#define SKML_DENSE_SEQ gradient_dense_x<skml_glm_dense_data, launch_glm_dense_predict, launch_glm_dense_plus_by>
#define SKML_LOWP_SEQ gradient_dense_x<skml_glm_dense_lowp_data, launch_glm_dense_lowp_predict, launch_glm_dense_lowp_plus_by>
SKML_GRADIENT_ENTRY(skml_glm_gradient_f64, skml_glm_data, double, gradient_x<false>)
SKML_GRADIENT_ENTRY(skml_glm_gradient_f32, skml_glm_data, float, gradient_x<false>)
SKML_GRADIENT_ENTRY(skml_glm_gradient_segmented_f64, skml_glm_data, double, gradient_x<true>)
SKML_GRADIENT_ENTRY(skml_glm_gradient_segmented_f32, skml_glm_data, float, gradient_x<true>)
SKML_GRADIENT_ENTRY(skml_glm_gradient_dense_f64, skml_glm_dense_data, double, SKML_DENSE_SEQ)
SKML_GRADIENT_ENTRY(skml_glm_gradient_dense_f32, skml_glm_dense_data, float, SKML_DENSE_SEQ)
SKML_GRADIENT_ENTRY(skml_glm_gradient_dense_lowp_f64, skml_glm_dense_lowp_data, double, SKML_LOWP_SEQ)
SKML_GRADIENT_ENTRY(skml_glm_gradient_dense_lowp_f32, skml_glm_dense_lowp_data, float, SKML_LOWP_SEQ)
SKML_GRADIENT_ENTRY(skml_glm_gradient_dense_blocked_f64, skml_glm_dense_data, double, gradient_dense_blocked_x)
SKML_GRADIENT_ENTRY(skml_glm_gradient_dense_blocked_f32, skml_glm_dense_data, float, gradient_dense_blocked_x)
SKML_GRADIENT_ENTRY(skml_glm_gradient_dense_lowp_blocked_f64, skml_glm_dense_lowp_data, double, gradient_dense_blocked_x)
SKML_GRADIENT_ENTRY(skml_glm_gradient_dense_lowp_blocked_f32, skml_glm_dense_lowp_data, float, gradient_dense_blocked_x)
SKML_GRADIENT_MULTI_ENTRY(skml_glm_gradient_dense_multi_f64, skml_glm_dense_data, double)
SKML_GRADIENT_MULTI_ENTRY(skml_glm_gradient_dense_multi_f32, skml_glm_dense_data, float)
SKML_GRADIENT_MULTI_ENTRY(skml_glm_gradient_dense_lowp_multi_f64, skml_glm_dense_lowp_data, double)
SKML_GRADIENT_MULTI_ENTRY(skml_glm_gradient_dense_lowp_multi_f32, skml_glm_dense_lowp_data, float)
#undef SKML_GRADIENT_ENTRY
#undef SKML_GRADIENT_MULTI_ENTRY
#undef SKML_DENSE_SEQ
#undef SKML_LOWP_SEQ

int skml_debug_glm_segmented_constant(int which) {
    switch (which) {
        case SKML_GLM_SEG_M_SEQ: return kSegMSeq;
        case SKML_GLM_SEG_SPLIT_AT: return kSegSplitAt;
        case SKML_GLM_SEG_SLICE: return kSegSlice;
        case SKML_GLM_SEG_TILE: return kSegTile;
        default: return -1;
    }
}

int skml_debug_glm_dense_blocked_plan(int x_bytes, int64_t batch, int64_t dim, int64_t out[6]) {
    BlkPlan p;
    if (!out || !blk_plan(x_bytes, batch, dim, &p)) return -1;
    out[0] = p.lanes;
    out[1] = p.split;
    out[2] = p.rows_in_flight;
    out[3] = p.rb;
    out[4] = p.nb;
    out[5] = p.ws_bytes;
    return 0;
}

int skml_debug_glm_dense_multi_plan(int x_bytes, int models, int64_t batch, int64_t dim, int64_t out[8]) {
    MulPlan p;
    if (!out || !mul_plan(x_bytes, models, batch, dim, &p)) return -1;
    out[0] = kMulTileRows;
    out[1] = p.tiles_per_wave;
    out[2] = p.split;
    out[3] = p.lane_cols;
    out[4] = p.strip_cols;
    out[5] = p.rb;
    out[6] = p.nb;
    out[7] = p.ws_bytes;
    return 0;
}

int skml_debug_glm_dense_lowp_constant(int x_kind, int which) {
    const int e = lowp_elems_per_group(x_kind);
    if (!e) return -1;
    switch (which) {
        case SKML_GLM_DENSE_C: return e == 4 ? LowpTile<4>::kC : LowpTile<8>::kC;
        case SKML_GLM_DENSE_STRIDE: return e == 4 ? LowpTile<4>::kS : LowpTile<8>::kS;
        case SKML_GLM_DENSE_U: return kLowpU;
        case SKML_GLM_DENSE_V: return e == 4 ? LowpCols<4>::kV : LowpCols<8>::kV;
        case SKML_GLM_DENSE_ROW_GROUP_AT: return (int)kLowpGroupAt;
        case SKML_GLM_DENSE_COL_GROUP_AT: return (int)kLowpColGroupAt;
        default: return -1;
    }
}

int skml_debug_glm_dense_constant(int which) {
    switch (which) {
        case SKML_GLM_DENSE_C: return kDenseC;
        case SKML_GLM_DENSE_STRIDE: return kDenseS;
        case SKML_GLM_DENSE_U: return kDenseU;
        case SKML_GLM_DENSE_V: return kDenseV;
        case SKML_GLM_DENSE_ROW_GROUP_AT: return (int)kDenseGroupAt;
        case SKML_GLM_DENSE_COL_GROUP_AT: return (int)kDenseColGroupAt;
        default: return -1;
    }
}

int skml_glm_finish_dense_f64(skml_ctx* c, double* g, int64_t dim, double times, int32_t reg_kind, double reg_param,
                              const void* w, int32_t w_fp32) {
    return finish_x(c, nullptr, false, g, dim, dim, times, reg_kind, reg_param, w, w_fp32);
}

int skml_glm_finish_kv_f64(skml_ctx* c, const int32_t* keys, double* vals, int64_t nnz, int64_t dim, double times,
                           int32_t reg_kind, double reg_param, const void* w, int32_t w_fp32) {
    return finish_x(c, keys, true, vals, nnz, dim, times, reg_kind, reg_param, w, w_fp32);
}

}  // extern "C"
