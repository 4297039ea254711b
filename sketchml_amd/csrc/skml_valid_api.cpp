// skml_valid_api.cpp -- host side of the validation pass of the C ABI (include/skml.h;
// ml/util/ValidationUtil.scala:12-93): argument checks, the context buffer that holds the counters, the
// stand-ins for the arrays the caller does not keep and the sort's scratch, the launches of
// skml_glm.hip / skml_valid.hip and the one read-back through pinned staging.
#include "skml_host.hpp"

using namespace skml;

namespace {

// The head of the workspace, read back as one block: counters [0 .. 5) of k_glm_valid (truePos, trueNeg,
// falsePos, falseNeg, NaN scores), [5] the sum's bits, [6] sigma, [7] M, [8] the NaN scores of k_valid_keys.
constexpr size_t kHeadWords = 9, kHead = 256;
static_assert(kHeadWords * 8 <= kHead, "the head holds its words");

// The AUC stage queued on the stream: keys, eight passes, the rank sum into head[6], head[7], head[8]
// (zeroed by the caller on the same stream).
int queue_auc(skml_ctx* c, const double* scores, const double* labels, int64_t n, int32_t* order, char* scratch,
              unsigned long long* head) {
    ValidAucScratch s;
    valid_auc_layout(n, &s, scratch);
    {
        KernelTimer kt(c, SKML_K_VALID_SORT);
        HIP_TRY(launch_valid_keys(c->stream, scores, n, s, head + 8));
    }
    for (int pass = 0; pass < 8; pass++) {
        KernelTimer kt(c, SKML_K_VALID_SORT);
        HIP_TRY(launch_valid_sort_pass(c->stream, n, pass, s));
    }
    KernelTimer kt(c, SKML_K_VALID_RANK);
    HIP_TRY(launch_valid_rank_sum(c->stream, s, labels, n, order, head + 6));
    return SKML_OK;
}

// The workspace: the head, then `extra` bytes of the caller's stand-ins, then the sort's scratch.
int valid_ws(skml_ctx* c, size_t extra, int64_t auc_n, char** base) {
    const size_t need = kHead + align_up(extra, 256) + (auc_n > 0 ? valid_auc_layout(auc_n, nullptr, nullptr) : 0);
    if (const int st = reserve(c, c->glm_ws, need, need + need / 4, "the validation pass's workspace")) return st;
    *base = static_cast<char*>(c->glm_ws.p);
    return SKML_OK;
}

int read_head(skml_ctx* c, const char* base, unsigned long long* words) {
    unsigned long long* pin = static_cast<unsigned long long*>(ctx_pinned(c, kHeadWords * 8));
    if (!pin) return fail(SKML_E_OOM, "pinned staging of the validation result");
    HIP_TRY(hipMemcpyAsync(pin, base, kHeadWords * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < kHeadWords; i++) words[i] = pin[i];
    return SKML_OK;
}

double as_double(unsigned long long bits) {
    double v;
    static_assert(sizeof(v) == sizeof(bits), "a sum travels as 8 bytes");
    __builtin_memcpy(&v, &bits, sizeof(v));
    return v;
}

int validate_x(skml_ctx* c, const skml_glm_data* d, int32_t loss_kind, const void* w, int wide, int32_t flags, double* pre_out,
               double* loss_out, skml_valid_result* out) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!d) return fail(SKML_E_ARG, "data is NULL");
    if (!out) return fail(SKML_E_ARG, "out is NULL");
    if (d->rows < 1 || d->rows > kJavaIntMax || d->dim < 1 || d->dim > kJavaIntMax || d->nnz < 0)
        return fail(SKML_E_ARG, "rows=%lld or dim=%lld outside [1, 2^31 - 1], or nnz=%lld < 0", (long long)d->rows,
                    (long long)d->dim, (long long)d->nnz);
    if (loss_kind != SKML_LOSS_L1_LOG && loss_kind != SKML_LOSS_L2_HINGE && loss_kind != SKML_LOSS_L2_LOG &&
        loss_kind != SKML_LOSS_L2_SQUARE)
        return fail(SKML_E_ARG, "unknown loss %d", loss_kind);
    if (flags & ~(SKML_VALID_AUC | SKML_VALID_TREE_SUM)) return fail(SKML_E_ARG, "unknown flag bits 0x%x", (unsigned)flags);
    const size_t nz = (size_t)d->nnz, rb = (size_t)d->rows * 8;
    const Range in[] = {{d->row_ptr, ((size_t)d->rows + 1) * 8, "row_ptr"}, {d->col, nz * 4, "col"}, {d->val, nz * 8, "val"},
                        {d->label, rb, "label"}, {w, (size_t)d->dim * (wide ? 8 : 4), "w"}};
    const Range outs[] = {{pre_out, rb, "pre_out"}, {loss_out, rb, "loss_out"}};
    if (!d->row_ptr || !d->label || !w) return fail(SKML_E_ARG, "row_ptr, label or w is NULL");
    if (nz && (!d->col || !d->val)) return fail(SKML_E_ARG, "col or val is NULL");
    for (const Range& r : in)
        if (!aligned8(r.p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", r.name);
    for (const Range& r : outs) {
        if (!aligned8(r.p)) return fail(SKML_E_ARG, "%s must be 8-byte aligned", r.name);
        for (const Range& q : in)
            if (overlap(r, q)) return fail(SKML_E_ARG, "%s and %s overlap", r.name, q.name);
    }
    if (overlap(outs[0], outs[1])) return fail(SKML_E_ARG, "pre_out and loss_out overlap");

    HIP_TRY(hipSetDevice(c->device));
    const bool auc = flags & SKML_VALID_AUC;
    const size_t extra = (pre_out || !auc ? 0 : align_up(rb, 256)) + (loss_out ? 0 : align_up(rb, 256));
    char* base = nullptr;
    if (const int st = valid_ws(c, extra, auc ? d->rows : 0, &base)) return st;
    unsigned long long* head = reinterpret_cast<unsigned long long*>(base);
    char* at = base + kHead;
    double* pre = pre_out;
    if (!pre && auc) {  // the sort reads the scores
        pre = reinterpret_cast<double*>(at);
        at += align_up(rb, 256);
    }
    double* loss = loss_out ? loss_out : reinterpret_cast<double*>(at);
    char* scratch = base + kHead + align_up(extra, 256);

    HIP_TRY(hipMemsetAsync(head, 0, kHead, c->stream));
    {
        KernelTimer kt(c, SKML_K_GLM_VALID);
        HIP_TRY(launch_glm_valid(c->stream, *d, loss_kind, w, wide, glm_lanes_per_row(d->nnz, d->rows), pre, loss, head));
    }
    {
        KernelTimer kt(c, SKML_K_SEQ_SUM);
        double* sum = reinterpret_cast<double*>(head + 5);
        if (flags & SKML_VALID_TREE_SUM) HIP_TRY(launch_glm_loss_sum(c->stream, loss, d->rows, sum));
        else HIP_TRY(launch_glm_seq_sum(c->stream, loss, d->rows, sum));
    }
    if (auc)
        if (const int st = queue_auc(c, pre, d->label, d->rows, nullptr, scratch, head)) return st;
    unsigned long long h[kHeadWords];
    if (const int st = read_head(c, base, h)) return st;
    skml_valid_result r;
    r.loss = as_double(h[5]);
    r.true_pos = (int64_t)h[0];
    r.true_neg = (int64_t)h[1];
    r.false_pos = (int64_t)h[2];
    r.false_neg = (int64_t)h[3];
    r.num = d->rows;
    r.pos = auc ? (int64_t)h[7] : 0;
    r.neg = auc ? d->rows - (int64_t)h[7] : 0;
    r.rank_sum = auc ? (uint64_t)h[6] : 0;
    r.nan_scores = (int64_t)h[4];
    *out = r;
    return SKML_OK;
}

}  // namespace

extern "C" {

int skml_glm_validate_f64(skml_ctx* c, const skml_glm_data* data, int32_t loss_kind, const double* w, int32_t flags,
                          double* pre_out, double* loss_out, skml_valid_result* out) {
    return validate_x(c, data, loss_kind, w, 1, flags, pre_out, loss_out, out);
}

int skml_glm_validate_f32(skml_ctx* c, const skml_glm_data* data, int32_t loss_kind, const float* w, int32_t flags,
                          double* pre_out, double* loss_out, skml_valid_result* out) {
    return validate_x(c, data, loss_kind, w, 0, flags, pre_out, loss_out, out);
}

int skml_auc_rank_sum(skml_ctx* c, const double* scores, const double* labels, int64_t n, int32_t* order_out, int64_t* pos,
                      int64_t* neg, uint64_t* rank_sum, int64_t* nan_scores) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (n < 1 || n > kJavaIntMax) return fail(SKML_E_ARG, "n=%lld outside [1, 2^31 - 1]", (long long)n);
    if (!scores || !labels) return fail(SKML_E_ARG, "scores or labels is NULL");
    if (!pos || !neg || !rank_sum || !nan_scores) return fail(SKML_E_ARG, "pos, neg, rank_sum or nan_scores is NULL");
    if (!aligned8(scores) || !aligned8(labels) || ((uintptr_t)order_out) % 4)
        return fail(SKML_E_ARG, "scores and labels must be 8-byte aligned, order_out 4-byte");
    const Range rs{scores, (size_t)n * 8, "scores"}, rl{labels, (size_t)n * 8, "labels"}, ro{order_out, (size_t)n * 4, "order_out"};
    if (overlap(ro, rs) || overlap(ro, rl)) return fail(SKML_E_ARG, "order_out overlaps scores or labels");
    HIP_TRY(hipSetDevice(c->device));
    char* base = nullptr;
    if (const int st = valid_ws(c, 0, n, &base)) return st;
    unsigned long long* head = reinterpret_cast<unsigned long long*>(base);
    HIP_TRY(hipMemsetAsync(head, 0, kHead, c->stream));
    if (const int st = queue_auc(c, scores, labels, n, order_out, base + kHead, head)) return st;
    unsigned long long h[kHeadWords];
    if (const int st = read_head(c, base, h)) return st;
    *pos = (int64_t)h[7];
    *neg = n - (int64_t)h[7];
    *rank_sum = (uint64_t)h[6];
    *nan_scores = (int64_t)h[8];
    return SKML_OK;
}

int skml_glm_seq_sum(skml_ctx* c, const double* x, int64_t n, double* sum) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (n < 1 || n > kJavaIntMax) return fail(SKML_E_ARG, "n=%lld outside [1, 2^31 - 1]", (long long)n);
    if (!x || !sum) return fail(SKML_E_ARG, "x or sum is NULL");
    if (!aligned8(x)) return fail(SKML_E_ARG, "x must be 8-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    char* base = nullptr;
    if (const int st = valid_ws(c, 0, 0, &base)) return st;
    unsigned long long* head = reinterpret_cast<unsigned long long*>(base);
    {
        KernelTimer kt(c, SKML_K_SEQ_SUM);
        HIP_TRY(launch_glm_seq_sum(c->stream, x, n, reinterpret_cast<double*>(head + 5)));
    }
    unsigned long long h[kHeadWords];
    if (const int st = read_head(c, base, h)) return st;
    *sum = as_double(h[5]);
    return SKML_OK;
}

}  // extern "C"
