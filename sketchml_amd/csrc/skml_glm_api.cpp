// skml_glm_api.cpp -- host side of the mini-batch gradient of the C ABI (include/skml.h;
// ml/objective/GradientDescent.scala:23-87): argument checks, the context buffer that stands in for
// the arrays the caller does not keep, the launches of skml_glm.hip and the one read-back of
// toAuto's count and objLoss.
#include "skml_glm_dense.hpp"
#include "skml_glm_dense_blocked.hpp"
#include "skml_glm_dense_multi.hpp"
#include "skml_glm_segmented.hpp"
#include "skml_host.hpp"

using namespace skml;

namespace {

constexpr size_t kGlmHead = 256;  // the live counter and objLoss, ahead of the stand-in arrays

// What the sparse and the dense gradient share once their arguments are checked: the workspace that
// stands in for coef / loss_j, predict(coef, loss), the loss sum, plus_by(coef, counter) and the one
// read-back of toAuto's count and objLoss after the one synchronisation.
template <typename Predict, typename PlusBy>
int gradient_run(skml_ctx* c, int64_t batch, double* coef_out, double* loss_out, int64_t* nnz_out, double* obj_loss_out,
                 Predict predict, PlusBy plus_by) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t bb = (size_t)batch * 8, need = kGlmHead + 2 * bb;
    if (const int st = reserve(c, c->glm_ws, need, need + need / 4, "the mini-batch gradient's workspace")) return st;
    char* base = static_cast<char*>(c->glm_ws.p);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(base);
    double* obj = reinterpret_cast<double*>(base + 8);
    double* coef = coef_out ? coef_out : reinterpret_cast<double*>(base + kGlmHead);
    double* loss = loss_out ? loss_out : reinterpret_cast<double*>(base + kGlmHead + bb);
    unsigned long long* pin = static_cast<unsigned long long*>(ctx_pinned(c, 16));
    if (!pin) return fail(SKML_E_OOM, "pinned staging of the live count and objLoss");

    HIP_TRY(hipMemsetAsync(cnt, 0, 16, c->stream));
    {
        KernelTimer kt(c, SKML_K_GLM_PREDICT);
        HIP_TRY(predict(coef, loss));
        HIP_TRY(launch_glm_loss_sum(c->stream, loss, batch, obj));
    }
    {
        KernelTimer kt(c, SKML_K_GLM_PLUS_BY);
        HIP_TRY(plus_by(coef, cnt));
    }
    HIP_TRY(hipMemcpyAsync(pin, cnt, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *nnz_out = (int64_t)pin[0];
    double o;
    static_assert(sizeof(o) == sizeof(pin[1]), "objLoss travels as 8 bytes");
    __builtin_memcpy(&o, &pin[1], sizeof(o));
    *obj_loss_out = o;
    return SKML_OK;
}

// segmented: the column sum of skml_glm_segmented.hip in place of k_glm_plus_by; its work list and partial
// sums live in the context's staging, grown inside plus_by as the blocked order's are.
int gradient_x(skml_ctx* c, const skml_glm_data* d, int64_t row0, int64_t batch, int32_t loss_kind, const void* w, int wide,
               double* pre_out, double* coef_out, double* loss_out, double* grad_out, int64_t* nnz_out,
               double* obj_loss_out, bool segmented = false) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    if (d->rows < 1 || d->rows > kJavaIntMax || d->dim < 1 || d->dim > kJavaIntMax || d->nnz < 0)
        return fail(SKML_E_ARG, "rows=%lld or dim=%lld outside [1, 2^31 - 1], or nnz=%lld < 0", (long long)d->rows,
                    (long long)d->dim, (long long)d->nnz);
    if (row0 < 0 || row0 >= d->rows) return fail(SKML_E_ARG, "row0=%lld outside [0, %lld)", (long long)row0, (long long)d->rows);
    if (batch < 1 || batch > d->rows)
        return fail(SKML_E_ARG, "batch=%lld outside [1, %lld]: a window wraps at most once", (long long)batch, (long long)d->rows);
    if (loss_kind != SKML_LOSS_L1_LOG && loss_kind != SKML_LOSS_L2_HINGE && loss_kind != SKML_LOSS_L2_LOG &&
        loss_kind != SKML_LOSS_L2_SQUARE)
        return fail(SKML_E_ARG, "unknown loss %d", loss_kind);
    const size_t nz = (size_t)d->nnz, bb = (size_t)batch * 8, db = (size_t)d->dim * 8;
    const Range in[] = {{d->row_ptr, ((size_t)d->rows + 1) * 8, "row_ptr"}, {d->col, nz * 4, "col"}, {d->val, nz * 8, "val"},
                        {d->label, (size_t)d->rows * 8, "label"}, {d->col_ptr, ((size_t)d->dim + 1) * 8, "col_ptr"},
                        {d->csc_row, nz * 4, "csc_row"}, {d->csc_val, nz * 8, "csc_val"},
                        {w, (size_t)d->dim * (wide ? 8 : 4), "w"}};
    const Range out[] = {{pre_out, bb, "pre_out"}, {coef_out, bb, "coef_out"}, {loss_out, bb, "loss_out"}};
    const Range grad{grad_out, db, "grad_out"};
    if (!d->row_ptr || !d->label || !d->col_ptr || !w || !grad_out) return fail(SKML_E_ARG, "row_ptr, label, col_ptr, w or grad_out is NULL");
    if (nz && (!d->col || !d->val || !d->csc_row || !d->csc_val)) return fail(SKML_E_ARG, "col, val, csc_row or csc_val is NULL");
    if (!nnz_out || !obj_loss_out) return fail(SKML_E_ARG, "nnz_out or obj_loss_out is NULL");
    for (const Range& r : in)
        if (!aligned8(r.p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", r.name);
    for (const Range& r : out)
        if (!aligned8(r.p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", r.name);
    if (!aligned8(grad_out)) return fail(SKML_E_ARG, "grad_out must be 8-byte aligned");
    for (const Range& r : in)
        if (overlap(grad, r)) return fail(SKML_E_ARG, "grad_out and %s overlap", r.name);
    for (const Range& r : out) {
        if (overlap(grad, r)) return fail(SKML_E_ARG, "grad_out and %s overlap", r.name);
        for (const Range& q : in)
            if (overlap(r, q)) return fail(SKML_E_ARG, "%s and %s overlap", r.name, q.name);
    }
    if (overlap(out[0], out[1]) || overlap(out[0], out[2]) || overlap(out[1], out[2]))
        return fail(SKML_E_ARG, "pre_out, coef_out and loss_out overlap");

    return gradient_run(
        c, batch, coef_out, loss_out, nnz_out, obj_loss_out,
        [&](double* coef, double* loss) {
            return launch_glm_predict(c->stream, *d, row0, batch, loss_kind, w, wide, glm_lanes_per_row(d->nnz, d->rows), pre_out, coef, loss);
        },
        [&](const double* coef, unsigned long long* cnt) {
            if (!segmented) return launch_glm_plus_by(c->stream, *d, row0, batch, coef, grad_out, cnt);
            const size_t need = (size_t)seg_stage_bytes(d->dim, d->nnz);
            if (reserve(c, c->stage, need, need + need / 4, "the segmented gradient's work list")) return hipErrorOutOfMemory;
            return launch_glm_segmented_plus_by(c->stream, *d, row0, batch, coef, c->stage.p, grad_out, cnt);
        });
}

// What the dense entries share once rows, dim and the xb bytes of x are checked: gradient_x's other checks,
// then the same gradient_run.
template <typename Predict, typename PlusBy>
int gradient_dense_rest(skml_ctx* c, int64_t rows, int64_t dim, const void* x, size_t xb, const double* label, int64_t row0,
                        int64_t batch, int32_t loss_kind, const void* w, int wide, double* pre_out, double* coef_out,
                        double* loss_out, double* grad_out, int64_t* nnz_out, double* obj_loss_out, Predict predict,
                        PlusBy plus_by) {
    if (row0 < 0 || row0 >= rows) return fail(SKML_E_ARG, "row0=%lld outside [0, %lld)", (long long)row0, (long long)rows);
    if (batch < 1 || batch > rows)
        return fail(SKML_E_ARG, "batch=%lld outside [1, %lld]: a window wraps at most once", (long long)batch, (long long)rows);
    if (loss_kind != SKML_LOSS_L1_LOG && loss_kind != SKML_LOSS_L2_HINGE && loss_kind != SKML_LOSS_L2_LOG &&
        loss_kind != SKML_LOSS_L2_SQUARE)
        return fail(SKML_E_ARG, "unknown loss %d", loss_kind);
    const size_t bb = (size_t)batch * 8, db = (size_t)dim * 8;
    const Range in[] = {{x, xb, "x"}, {label, (size_t)rows * 8, "label"}, {w, (size_t)dim * (wide ? 8 : 4), "w"}};
    const Range out[] = {{pre_out, bb, "pre_out"}, {coef_out, bb, "coef_out"}, {loss_out, bb, "loss_out"}};
    const Range grad{grad_out, db, "grad_out"};
    if (!x || !label || !w || !grad_out) return fail(SKML_E_ARG, "x, label, w or grad_out is NULL");
    if (!nnz_out || !obj_loss_out) return fail(SKML_E_ARG, "nnz_out or obj_loss_out is NULL");
    for (const Range& r : in)
        if (!aligned8(r.p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", r.name);
    for (const Range& r : out)
        if (!aligned8(r.p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", r.name);
    if (!aligned8(grad_out)) return fail(SKML_E_ARG, "grad_out must be 8-byte aligned");
    for (const Range& r : in)
        if (overlap(grad, r)) return fail(SKML_E_ARG, "grad_out and %s overlap", r.name);
    for (const Range& r : out) {
        if (overlap(grad, r)) return fail(SKML_E_ARG, "grad_out and %s overlap", r.name);
        for (const Range& q : in)
            if (overlap(r, q)) return fail(SKML_E_ARG, "%s and %s overlap", r.name, q.name);
    }
    if (overlap(out[0], out[1]) || overlap(out[0], out[2]) || overlap(out[1], out[2]))
        return fail(SKML_E_ARG, "pre_out, coef_out and loss_out overlap");

    return gradient_run(c, batch, coef_out, loss_out, nnz_out, obj_loss_out, predict, plus_by);
}

// gradient_x over dense instances.
int gradient_dense_x(skml_ctx* c, const skml_glm_dense_data* d, int64_t row0, int64_t batch, int32_t loss_kind, const void* w,
                     int wide, double* pre_out, double* coef_out, double* loss_out, double* grad_out, int64_t* nnz_out,
                     double* obj_loss_out) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    if (d->rows < 1 || d->rows > kJavaIntMax || d->dim < 1 || d->dim > kJavaIntMax)
        return fail(SKML_E_ARG, "rows=%lld or dim=%lld outside [1, 2^31 - 1]", (long long)d->rows, (long long)d->dim);
    size_t xb = 0;
    if (!dense_bytes(d->rows, d->dim, &xb))
        return fail(SKML_E_ARG, "rows=%lld times dim=%lld doubles do not fit an int64", (long long)d->rows, (long long)d->dim);
    return gradient_dense_rest(
        c, d->rows, d->dim, d->x, xb, d->label, row0, batch, loss_kind, w, wide, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out,
        [&](double* coef, double* loss) { return launch_glm_dense_predict(c->stream, *d, row0, batch, loss_kind, w, wide, pre_out, coef, loss); },
        [&](const double* coef, unsigned long long* cnt) { return launch_glm_dense_plus_by(c->stream, *d, row0, batch, coef, grad_out, cnt); });
}

// gradient_dense_x over an x stored as fp32, bf16 or fp16.
int gradient_dense_lowp_x(skml_ctx* c, const skml_glm_dense_lowp_data* d, int64_t row0, int64_t batch, int32_t loss_kind,
                          const void* w, int wide, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                          int64_t* nnz_out, double* obj_loss_out) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    size_t xb = 0;
    if (const int st = dense_lowp_check(d, &xb)) return st;
    return gradient_dense_rest(
        c, d->rows, d->dim, d->x, xb, d->label, row0, batch, loss_kind, w, wide, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out,
        [&](double* coef, double* loss) { return launch_glm_dense_lowp_predict(c->stream, *d, row0, batch, loss_kind, w, wide, pre_out, coef, loss); },
        [&](const double* coef, unsigned long long* cnt) { return launch_glm_dense_lowp_plus_by(c->stream, *d, row0, batch, coef, grad_out, cnt); });
}

// The dense entries in the blocked summation order (skml_glm_dense_blocked.hip), once the struct is checked:
// gradient_dense_rest's checks come first, as for the sequential twins, and nothing is touched before them.
// The partial sums of the column sum live in the context's staging buffer, grown inside plus_by: every use of
// that buffer is ordered on the context's stream, and gradient_run's own workspace is not moved under it.
int gradient_dense_blocked_rest(skml_ctx* c, const GlmBlockedX& bx, int x_bytes, size_t xb, int64_t row0, int64_t batch,
                                int32_t loss_kind, const void* w, int wide, double* pre_out, double* coef_out, double* loss_out,
                                double* grad_out, int64_t* nnz_out, double* obj_loss_out) {
    return gradient_dense_rest(
        c, bx.rows, bx.dim, bx.x, xb, bx.label, row0, batch, loss_kind, w, wide, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out,
        [&](double* coef, double* loss) { return launch_glm_dense_blocked_predict(c->stream, bx, row0, batch, loss_kind, w, wide, pre_out, coef, loss); },
        [&](const double* coef, unsigned long long* cnt) {
            BlkPlan plan;
            if (!blk_plan(x_bytes, batch, bx.dim, &plan)) return hipErrorInvalidValue;
            const size_t need = (size_t)plan.ws_bytes;
            if (need && reserve(c, c->stage, need, need + need / 4, "the blocked gradient's partial sums")) return hipErrorOutOfMemory;
            return launch_glm_dense_blocked_plus_by(c->stream, bx, row0, batch, coef, need ? static_cast<double*>(c->stage.p) : nullptr,
                                                    grad_out, cnt);
        });
}

// gradient_dense_x in the blocked order.
int gradient_dense_blocked_x(skml_ctx* c, const skml_glm_dense_data* d, int64_t row0, int64_t batch, int32_t loss_kind,
                             const void* w, int wide, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                             int64_t* nnz_out, double* obj_loss_out) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    if (d->rows < 1 || d->rows > kJavaIntMax || d->dim < 1 || d->dim > kJavaIntMax)
        return fail(SKML_E_ARG, "rows=%lld or dim=%lld outside [1, 2^31 - 1]", (long long)d->rows, (long long)d->dim);
    size_t xb = 0;
    if (!dense_bytes(d->rows, d->dim, &xb))
        return fail(SKML_E_ARG, "rows=%lld times dim=%lld doubles do not fit an int64", (long long)d->rows, (long long)d->dim);
    const GlmBlockedX bx{d->rows, d->dim, d->dim, d->x, d->label, kBlkXF64};
    return gradient_dense_blocked_rest(c, bx, 8, xb, row0, batch, loss_kind, w, wide, pre_out, coef_out, loss_out, grad_out, nnz_out,
                                       obj_loss_out);
}

// gradient_dense_lowp_x in the blocked order.
int gradient_dense_lowp_blocked_x(skml_ctx* c, const skml_glm_dense_lowp_data* d, int64_t row0, int64_t batch, int32_t loss_kind,
                                  const void* w, int wide, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                                  int64_t* nnz_out, double* obj_loss_out) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    size_t xb = 0;
    if (const int st = dense_lowp_check(d, &xb)) return st;
    const GlmBlockedX bx{d->rows, d->dim, d->pitch, d->x, d->label, d->x_kind};
    return gradient_dense_blocked_rest(c, bx, 16 / lowp_elems_per_group(d->x_kind), xb, row0, batch, loss_kind, w, wide, pre_out, coef_out,
                                       loss_out, grad_out, nnz_out, obj_loss_out);
}

// The dense gradient of K <= 16 models in one pass over x (skml_glm_dense_multi.hip), once the struct is checked.
// A sibling of gradient_dense_rest and gradient_run, which serve one model: the checks are theirs in their order
// with K-fold ranges, the workspace holds K live counters and K objLoss (the same 256-byte head) ahead of the
// K x batch stand-ins, and the one read-back brings 2 K scalars.  The partial sums live in the context's staging
// buffer, reserved inside the column sum's step, after every check, as the blocked entries do.
int gradient_dense_multi_rest(skml_ctx* c, const GlmBlockedX& bx, int x_bytes, size_t xb, int64_t row0, int64_t batch, int32_t loss_kind,
                              int32_t models, const void* w, int wide, const double* labels, double* pre_out, double* coef_out,
                              double* loss_out, double* grad_out, int64_t* nnz_out, double* obj_loss_out) {
    const int64_t rows = bx.rows, dim = bx.dim;
    if (row0 < 0 || row0 >= rows) return fail(SKML_E_ARG, "row0=%lld outside [0, %lld)", (long long)row0, (long long)rows);
    if (batch < 1 || batch > rows)
        return fail(SKML_E_ARG, "batch=%lld outside [1, %lld]: a window wraps at most once", (long long)batch, (long long)rows);
    if (loss_kind != SKML_LOSS_L1_LOG && loss_kind != SKML_LOSS_L2_HINGE && loss_kind != SKML_LOSS_L2_LOG &&
        loss_kind != SKML_LOSS_L2_SQUARE)
        return fail(SKML_E_ARG, "unknown loss %d", loss_kind);
    if (models < 1 || models > kMulMaxModels) return fail(SKML_E_ARG, "models=%d outside [1, %d]", models, kMulMaxModels);
    int64_t kb = 0, kd = 0, kr = 0;
    if (!mul_bytes(models, batch, &kb) || !mul_bytes(models, dim, &kd) || !mul_bytes(models, rows, &kr))
        return fail(SKML_E_ARG, "models=%d times batch, dim or rows doubles do not fit an int64", models);
    const size_t bb = (size_t)kb, db = (size_t)kd;
    const Range in[] = {{bx.x, xb, "x"}, {bx.label, (size_t)rows * 8, "label"}, {w, wide ? db : db / 2, "w"}, {labels, (size_t)kr, "labels"}};
    const Range out[] = {{pre_out, bb, "pre_out"}, {coef_out, bb, "coef_out"}, {loss_out, bb, "loss_out"}};
    const Range grad{grad_out, db, "grad_out"};
    if (!bx.x || !bx.label || !w || !grad_out) return fail(SKML_E_ARG, "x, label, w or grad_out is NULL");
    if (!nnz_out || !obj_loss_out) return fail(SKML_E_ARG, "nnz_out or obj_loss_out is NULL");
    for (const Range& r : in)
        if (!aligned8(r.p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", r.name);
    for (const Range& r : out)
        if (!aligned8(r.p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", r.name);
    if (!aligned8(grad_out)) return fail(SKML_E_ARG, "grad_out must be 8-byte aligned");
    for (const Range& r : in)
        if (overlap(grad, r)) return fail(SKML_E_ARG, "grad_out and %s overlap", r.name);
    for (const Range& r : out) {
        if (overlap(grad, r)) return fail(SKML_E_ARG, "grad_out and %s overlap", r.name);
        for (const Range& q : in)
            if (overlap(r, q)) return fail(SKML_E_ARG, "%s and %s overlap", r.name, q.name);
    }
    if (overlap(out[0], out[1]) || overlap(out[0], out[2]) || overlap(out[1], out[2]))
        return fail(SKML_E_ARG, "pre_out, coef_out and loss_out overlap");
    MulPlan plan;
    if (!mul_plan(x_bytes, models, batch, dim, &plan)) return fail(SKML_E_ARG, "no plan for %d models, batch=%lld, dim=%lld", models, (long long)batch, (long long)dim);

    HIP_TRY(hipSetDevice(c->device));
    static_assert(kGlmHead >= 16 * kMulMaxModels, "K live counters and K objLoss ahead of the stand-in arrays");
    const size_t need = kGlmHead + 2 * bb;
    if (const int st = reserve(c, c->glm_ws, need, need + need / 4, "the mini-batch gradient's workspace")) return st;
    char* base = static_cast<char*>(c->glm_ws.p);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(base);
    double* obj = reinterpret_cast<double*>(base + 8 * kMulMaxModels);
    double* coef = coef_out ? coef_out : reinterpret_cast<double*>(base + kGlmHead);
    double* loss = loss_out ? loss_out : reinterpret_cast<double*>(base + kGlmHead + bb);
    unsigned long long* pin = static_cast<unsigned long long*>(ctx_pinned(c, kGlmHead));
    if (!pin) return fail(SKML_E_OOM, "pinned staging of the live counts and objLoss");

    HIP_TRY(hipMemsetAsync(base, 0, kGlmHead, c->stream));
    {
        KernelTimer kt(c, SKML_K_GLM_PREDICT);
        HIP_TRY(launch_glm_dense_multi_predict(c->stream, bx, row0, batch, loss_kind, w, wide, models, labels, pre_out, coef, loss));
        HIP_TRY(launch_glm_dense_multi_loss_sum(c->stream, loss, batch, models, obj));
    }
    {
        KernelTimer kt(c, SKML_K_GLM_PLUS_BY);
        const size_t ws = (size_t)plan.ws_bytes;
        if (ws)
            if (const int st = reserve(c, c->stage, ws, ws + ws / 4, "the multi-model gradient's partial sums")) return st;
        HIP_TRY(launch_glm_dense_multi_plus_by(c->stream, bx, row0, batch, coef, models, ws ? static_cast<double*>(c->stage.p) : nullptr,
                                               grad_out, cnt));
    }
    HIP_TRY(hipMemcpyAsync(pin, base, kGlmHead, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int m = 0; m < models; m++) {
        nnz_out[m] = (int64_t)pin[m];
        __builtin_memcpy(&obj_loss_out[m], &pin[kMulMaxModels + m], 8);
    }
    return SKML_OK;
}

// gradient_dense_blocked_x for K models.
int gradient_dense_multi_x(skml_ctx* c, const skml_glm_dense_data* d, int64_t row0, int64_t batch, int32_t loss_kind, int32_t models,
                           const void* w, int wide, const double* labels, double* pre_out, double* coef_out, double* loss_out,
                           double* grad_out, int64_t* nnz_out, double* obj_loss_out) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    if (d->rows < 1 || d->rows > kJavaIntMax || d->dim < 1 || d->dim > kJavaIntMax)
        return fail(SKML_E_ARG, "rows=%lld or dim=%lld outside [1, 2^31 - 1]", (long long)d->rows, (long long)d->dim);
    size_t xb = 0;
    if (!dense_bytes(d->rows, d->dim, &xb))
        return fail(SKML_E_ARG, "rows=%lld times dim=%lld doubles do not fit an int64", (long long)d->rows, (long long)d->dim);
    const GlmBlockedX bx{d->rows, d->dim, d->dim, d->x, d->label, kBlkXF64};
    return gradient_dense_multi_rest(c, bx, 8, xb, row0, batch, loss_kind, models, w, wide, labels, pre_out, coef_out, loss_out, grad_out,
                                     nnz_out, obj_loss_out);
}

// gradient_dense_lowp_blocked_x for K models.
int gradient_dense_lowp_multi_x(skml_ctx* c, const skml_glm_dense_lowp_data* d, int64_t row0, int64_t batch, int32_t loss_kind,
                                int32_t models, const void* w, int wide, const double* labels, double* pre_out, double* coef_out,
                                double* loss_out, double* grad_out, int64_t* nnz_out, double* obj_loss_out) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    size_t xb = 0;
    if (const int st = dense_lowp_check(d, &xb)) return st;
    const GlmBlockedX bx{d->rows, d->dim, d->pitch, d->x, d->label, d->x_kind};
    return gradient_dense_multi_rest(c, bx, 16 / lowp_elems_per_group(d->x_kind), xb, row0, batch, loss_kind, models, w, wide, labels, pre_out,
                                     coef_out, loss_out, grad_out, nnz_out, obj_loss_out);
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

int skml_glm_gradient_f64(skml_ctx* c, const skml_glm_data* data, int64_t row0, int64_t batch, int32_t loss_kind,
                          const double* w, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                          int64_t* nnz_out, double* obj_loss_out) {
    return gradient_x(c, data, row0, batch, loss_kind, w, 1, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out);
}

int skml_glm_gradient_f32(skml_ctx* c, const skml_glm_data* data, int64_t row0, int64_t batch, int32_t loss_kind,
                          const float* w, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                          int64_t* nnz_out, double* obj_loss_out) {
    return gradient_x(c, data, row0, batch, loss_kind, w, 0, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out);
}

int skml_glm_gradient_dense_f64(skml_ctx* c, const skml_glm_dense_data* data, int64_t row0, int64_t batch, int32_t loss_kind,
                                const double* w, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                                int64_t* nnz_out, double* obj_loss_out) {
    return gradient_dense_x(c, data, row0, batch, loss_kind, w, 1, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out);
}

int skml_glm_gradient_dense_f32(skml_ctx* c, const skml_glm_dense_data* data, int64_t row0, int64_t batch, int32_t loss_kind,
                                const float* w, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                                int64_t* nnz_out, double* obj_loss_out) {
    return gradient_dense_x(c, data, row0, batch, loss_kind, w, 0, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out);
}

int skml_glm_gradient_dense_lowp_f64(skml_ctx* c, const skml_glm_dense_lowp_data* data, int64_t row0, int64_t batch,
                                     int32_t loss_kind, const double* w, double* pre_out, double* coef_out, double* loss_out,
                                     double* grad_out, int64_t* nnz_out, double* obj_loss_out) {
    return gradient_dense_lowp_x(c, data, row0, batch, loss_kind, w, 1, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out);
}

int skml_glm_gradient_dense_lowp_f32(skml_ctx* c, const skml_glm_dense_lowp_data* data, int64_t row0, int64_t batch,
                                     int32_t loss_kind, const float* w, double* pre_out, double* coef_out, double* loss_out,
                                     double* grad_out, int64_t* nnz_out, double* obj_loss_out) {
    return gradient_dense_lowp_x(c, data, row0, batch, loss_kind, w, 0, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out);
}

int skml_glm_gradient_segmented_f64(skml_ctx* c, const skml_glm_data* data, int64_t row0, int64_t batch, int32_t loss_kind,
                                    const double* w, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                                    int64_t* nnz_out, double* obj_loss_out) {
    return gradient_x(c, data, row0, batch, loss_kind, w, 1, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out, true);
}

int skml_glm_gradient_segmented_f32(skml_ctx* c, const skml_glm_data* data, int64_t row0, int64_t batch, int32_t loss_kind,
                                    const float* w, double* pre_out, double* coef_out, double* loss_out, double* grad_out,
                                    int64_t* nnz_out, double* obj_loss_out) {
    return gradient_x(c, data, row0, batch, loss_kind, w, 0, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out, true);
}

int skml_debug_glm_segmented_constant(int which) {
    switch (which) {
        case SKML_GLM_SEG_M_SEQ: return kSegMSeq;
        case SKML_GLM_SEG_SPLIT_AT: return kSegSplitAt;
        case SKML_GLM_SEG_SLICE: return kSegSlice;
        case SKML_GLM_SEG_TILE: return kSegTile;
        default: return -1;
    }
}

#define SKML_BLOCKED_ENTRY(name, data_t, w_t, fn, wide)                                                                              \
    int name(skml_ctx* c, const data_t* data, int64_t row0, int64_t batch, int32_t loss_kind, const w_t* w, double* pre_out,         \
             double* coef_out, double* loss_out, double* grad_out, int64_t* nnz_out, double* obj_loss_out) {                         \
        return fn(c, data, row0, batch, loss_kind, w, wide, pre_out, coef_out, loss_out, grad_out, nnz_out, obj_loss_out);           \
    }
SKML_BLOCKED_ENTRY(skml_glm_gradient_dense_blocked_f64, skml_glm_dense_data, double, gradient_dense_blocked_x, 1)
SKML_BLOCKED_ENTRY(skml_glm_gradient_dense_blocked_f32, skml_glm_dense_data, float, gradient_dense_blocked_x, 0)
SKML_BLOCKED_ENTRY(skml_glm_gradient_dense_lowp_blocked_f64, skml_glm_dense_lowp_data, double, gradient_dense_lowp_blocked_x, 1)
SKML_BLOCKED_ENTRY(skml_glm_gradient_dense_lowp_blocked_f32, skml_glm_dense_lowp_data, float, gradient_dense_lowp_blocked_x, 0)
#undef SKML_BLOCKED_ENTRY

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

#define SKML_MULTI_ENTRY(name, data_t, w_t, fn, wide)                                                                                \
    int name(skml_ctx* c, const data_t* data, int64_t row0, int64_t batch, int32_t loss_kind, int32_t models, const w_t* w,          \
             const double* labels, double* pre_out, double* coef_out, double* loss_out, double* grad_out, int64_t* nnz_out,          \
             double* obj_loss_out) {                                                                                                 \
        return fn(c, data, row0, batch, loss_kind, models, w, wide, labels, pre_out, coef_out, loss_out, grad_out, nnz_out,          \
                  obj_loss_out);                                                                                                     \
    }
SKML_MULTI_ENTRY(skml_glm_gradient_dense_multi_f64, skml_glm_dense_data, double, gradient_dense_multi_x, 1)
SKML_MULTI_ENTRY(skml_glm_gradient_dense_multi_f32, skml_glm_dense_data, float, gradient_dense_multi_x, 0)
SKML_MULTI_ENTRY(skml_glm_gradient_dense_lowp_multi_f64, skml_glm_dense_lowp_data, double, gradient_dense_lowp_multi_x, 1)
SKML_MULTI_ENTRY(skml_glm_gradient_dense_lowp_multi_f32, skml_glm_dense_lowp_data, float, gradient_dense_lowp_multi_x, 0)
#undef SKML_MULTI_ENTRY

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
