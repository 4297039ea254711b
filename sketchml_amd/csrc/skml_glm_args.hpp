// skml_glm_args.hpp -- the argument checks of the mini-batch gradient and the validation entries
// (skml_glm_api.cpp, skml_valid_api.cpp), each written once: the data structs' heads, the window, the loss, and
// the alignment and overlap of the callers' arrays.  Nothing here touches a device or dereferences a pointer, and
// no HIP header is included: tests/glm_args_check.cpp runs the checks on the host over made-up addresses.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/skml.h"
#include "skml_glm_dense_lowp.hpp"
#include "skml_glm_dense_multi.hpp"

namespace skml {

// Sets the calling thread's skml_last_error message and returns `code` (skml_ctx.cpp).
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// A named byte range of a caller's array (a NULL or empty range overlaps nothing), 8-byte alignment, and the
// largest length a Java int holds.
struct Range {
    const void* p;
    size_t bytes;
    const char* name;
};
inline bool overlap(const Range& a, const Range& b) {
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
inline bool aligned8(const void* p) { return ((uintptr_t)p) % 8 == 0; }
constexpr int64_t kJavaIntMax = 0x7FFFFFFFLL;

// The arrays a gradient entry writes: pre, coef and loss may be NULL (nobody keeps them), the rest may not.
struct GlmOut {
    double *pre, *coef, *loss, *grad;
    int64_t* nnz;
    double* obj_loss;
};

// Every `in` (read), `out` (written, may be NULL) and `grad` (written, or nullptr for an entry without one) is
// 8-byte aligned, and nothing written overlaps anything else.
inline int ranges_check(const Range* in, int n_in, const Range* out, int n_out, const Range* grad) {
    const Range* sets[] = {in, out, grad};
    const int counts[] = {n_in, n_out, grad ? 1 : 0};
    for (int s = 0; s < 3; s++)
        for (int i = 0; i < counts[s]; i++)
            if (!aligned8(sets[s][i].p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", sets[s][i].name);
    for (int i = 0; grad && i < n_in; i++)
        if (overlap(*grad, in[i])) return fail(SKML_E_ARG, "%s and %s overlap", grad->name, in[i].name);
    for (int i = 0; i < n_out; i++) {
        if (grad && overlap(*grad, out[i])) return fail(SKML_E_ARG, "%s and %s overlap", grad->name, out[i].name);
        for (int j = 0; j < n_in; j++)
            if (overlap(out[i], in[j])) return fail(SKML_E_ARG, "%s and %s overlap", out[i].name, in[j].name);
    }
    for (int i = 0; i < n_out; i++)
        for (int j = i + 1; j < n_out; j++)
            if (overlap(out[i], out[j])) return fail(SKML_E_ARG, "%s and %s overlap", out[i].name, out[j].name);
    return SKML_OK;
}

inline int loss_check(int32_t loss_kind) {
    if (loss_kind != SKML_LOSS_L1_LOG && loss_kind != SKML_LOSS_L2_HINGE && loss_kind != SKML_LOSS_L2_LOG &&
        loss_kind != SKML_LOSS_L2_SQUARE)
        return fail(SKML_E_ARG, "unknown loss %d", loss_kind);
    return SKML_OK;
}

// The rows (row0 + j) mod rows, j < batch, of loopingRead.
inline int window_check(int64_t rows, int64_t row0, int64_t batch) {
    if (row0 < 0 || row0 >= rows) return fail(SKML_E_ARG, "row0=%lld outside [0, %lld)", (long long)row0, (long long)rows);
    if (batch < 1 || batch > rows)
        return fail(SKML_E_ARG, "batch=%lld outside [1, %lld]: a window wraps at most once", (long long)batch, (long long)rows);
    return SKML_OK;
}

// ---- what the entries over each data struct check of the struct before anything else ----
inline int sparse_check(const skml_glm_data* d) {
    if (d->rows < 1 || d->rows > kJavaIntMax || d->dim < 1 || d->dim > kJavaIntMax || d->nnz < 0)
        return fail(SKML_E_ARG, "rows=%lld or dim=%lld outside [1, 2^31 - 1], or nnz=%lld < 0", (long long)d->rows,
                    (long long)d->dim, (long long)d->nnz);
    return SKML_OK;
}

// *bytes of the rows * dim doubles of a dense data set; false when rows * dim * 8 does not fit an int64
inline bool dense_bytes(int64_t rows, int64_t dim, size_t* bytes) {
    int64_t n;
    if (__builtin_mul_overflow(rows, dim, &n) || n > INT64_MAX / 8) return false;
    *bytes = (size_t)n * 8;
    return true;
}

// rows and dim, and *bytes of x.
inline int dense_check(const skml_glm_dense_data* d, size_t* bytes) {
    if (d->rows < 1 || d->rows > kJavaIntMax || d->dim < 1 || d->dim > kJavaIntMax)
        return fail(SKML_E_ARG, "rows=%lld or dim=%lld outside [1, 2^31 - 1]", (long long)d->rows, (long long)d->dim);
    if (!dense_bytes(d->rows, d->dim, bytes))
        return fail(SKML_E_ARG, "rows=%lld times dim=%lld doubles do not fit an int64", (long long)d->rows, (long long)d->dim);
    return SKML_OK;
}

// rows and dim, the kind, the pitch rule, and *bytes of the rows * pitch elements of x.
inline int dense_lowp_check(const skml_glm_dense_lowp_data* d, size_t* bytes) {
    if (d->rows < 1 || d->rows > kJavaIntMax || d->dim < 1 || d->dim > kJavaIntMax)
        return fail(SKML_E_ARG, "rows=%lld or dim=%lld outside [1, 2^31 - 1]", (long long)d->rows, (long long)d->dim);
    const int64_t e = lowp_elems_per_group(d->x_kind);
    if (!e) return fail(SKML_E_ARG, "unknown x_kind %d", d->x_kind);
    if (d->pitch < d->dim || d->pitch % e)
        return fail(SKML_E_ARG, "pitch=%lld is below dim=%lld or leaves a row off a 16-byte boundary (a multiple of %lld elements)",
                    (long long)d->pitch, (long long)d->dim, (long long)e);
    if (((uintptr_t)d->x) % 16) return fail(SKML_E_ARG, "x must be 16-byte aligned");
    int64_t n;
    if (__builtin_mul_overflow(d->rows, d->pitch, &n) || n > INT64_MAX / (16 / e))
        return fail(SKML_E_ARG, "rows=%lld times pitch=%lld elements do not fit an int64", (long long)d->rows, (long long)d->pitch);
    *bytes = (size_t)n * (size_t)(16 / e);
    return SKML_OK;
}

// What the dense gradient entries check once the struct is: the window, the loss, K = models (1 for the
// single-model entries, whose labels is NULL) and the callers' arrays, model-major and K-fold where there is one
// per model: w K x dim, labels K x rows, pre / coef / loss K x batch, grad K x dim.
inline int dense_gradient_check(int64_t rows, int64_t dim, const void* x, size_t x_bytes, const double* label, int64_t row0,
                                int64_t batch, int32_t loss_kind, int32_t models, const void* w, int wide, const double* labels,
                                const GlmOut& o) {
    if (const int st = window_check(rows, row0, batch)) return st;
    if (const int st = loss_check(loss_kind)) return st;
    if (models < 1 || models > kMulMaxModels) return fail(SKML_E_ARG, "models=%d outside [1, %d]", models, kMulMaxModels);
    int64_t kb = 0, kd = 0, kr = 0;
    if (!mul_bytes(models, batch, &kb) || !mul_bytes(models, dim, &kd) || !mul_bytes(models, rows, &kr))
        return fail(SKML_E_ARG, "models=%d times batch, dim or rows doubles do not fit an int64", models);
    const size_t bb = (size_t)kb;
    const Range in[] = {{x, x_bytes, "x"}, {label, (size_t)rows * 8, "label"},
                        {w, (size_t)models * (size_t)dim * (wide ? 8 : 4), "w"}, {labels, (size_t)kr, "labels"}};
    const Range out[] = {{o.pre, bb, "pre_out"}, {o.coef, bb, "coef_out"}, {o.loss, bb, "loss_out"}};
    const Range grad{o.grad, (size_t)kd, "grad_out"};
    if (!x || !label || !w || !o.grad) return fail(SKML_E_ARG, "x, label, w or grad_out is NULL");
    if (!o.nnz || !o.obj_loss) return fail(SKML_E_ARG, "nnz_out or obj_loss_out is NULL");
    return ranges_check(in, 4, out, 3, &grad);
}

}  // namespace skml
