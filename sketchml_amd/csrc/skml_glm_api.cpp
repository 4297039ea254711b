// skml_glm_api.cpp -- host side of the mini-batch gradient of the C ABI (include/skml.h;
// ml/objective/GradientDescent.scala:23-87): argument checks, the context buffer that stands in for
// the arrays the caller does not keep, the launches of skml_glm.hip and the one read-back of
// toAuto's count and objLoss.
#include "skml_host.hpp"

using namespace skml;

namespace {

constexpr size_t kGlmHead = 256;  // the live counter and objLoss, ahead of the stand-in arrays

int gradient_x(skml_ctx* c, const skml_glm_data* d, int64_t row0, int64_t batch, int32_t loss_kind, const void* w, int wide,
               double* pre_out, double* coef_out, double* loss_out, double* grad_out, int64_t* nnz_out,
               double* obj_loss_out) {
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

    HIP_TRY(hipSetDevice(c->device));
    const size_t need = kGlmHead + 2 * bb;
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
        HIP_TRY(launch_glm_predict(c->stream, *d, row0, batch, loss_kind, w, wide, glm_lanes_per_row(d->nnz, d->rows), pre_out,
                                   coef, loss));
        HIP_TRY(launch_glm_loss_sum(c->stream, loss, batch, obj));
    }
    {
        KernelTimer kt(c, SKML_K_GLM_PLUS_BY);
        HIP_TRY(launch_glm_plus_by(c->stream, *d, row0, batch, coef, grad_out, cnt));
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

int skml_glm_finish_dense_f64(skml_ctx* c, double* g, int64_t dim, double times, int32_t reg_kind, double reg_param,
                              const void* w, int32_t w_fp32) {
    return finish_x(c, nullptr, false, g, dim, dim, times, reg_kind, reg_param, w, w_fp32);
}

int skml_glm_finish_kv_f64(skml_ctx* c, const int32_t* keys, double* vals, int64_t nnz, int64_t dim, double times,
                           int32_t reg_kind, double reg_param, const void* w, int32_t w_fp32) {
    return finish_x(c, keys, true, vals, nnz, dim, times, reg_kind, reg_param, w, w_fp32);
}

}  // extern "C"
