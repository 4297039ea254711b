// skml_optim_api.cpp -- host side of the optimiser update of the C ABI (include/skml.h;
// ml/objective/GradientDescent.scala:89-117, ml/objective/Adam.scala:27-77): argument checks, the
// step's constants, toAuto's count, and the launches of skml_optim.hip.
#include <cmath>
#include <cstring>

#include "skml_host.hpp"

using namespace skml;

namespace {

// The checks every entry shares, none of which needs a device: the context, the parameters, the
// state pointers (16-byte aligned, m and v exactly when Adam), and no two of `r` overlapping.
// r[0..3) are w, m, v; the entry appends its inputs.
int check_common(skml_ctx* c, const skml_opt_params* p, Range* r, int nr) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (!p) return fail(SKML_E_ARG, "params is NULL");
    if (p->kind != SKML_OPT_SGD && p->kind != SKML_OPT_ADAM) return fail(SKML_E_ARG, "unknown optimiser kind %d", p->kind);
    if (p->select != SKML_OPT_ALL && p->select != SKML_OPT_LIVE && p->select != SKML_OPT_AUTO)
        return fail(SKML_E_ARG, "unknown selection %d", p->select);
    if (!std::isfinite(p->lr)) return fail(SKML_E_ARG, "lr is not finite");
    if (p->kind == SKML_OPT_ADAM && !(std::isfinite(p->beta1) && std::isfinite(p->beta2) && std::isfinite(p->beta1_t) &&
                                      std::isfinite(p->beta2_t) && std::isfinite(p->eps)))
        return fail(SKML_E_ARG, "beta1, beta2, beta1_t, beta2_t and eps must be finite");
    if (!r[0].p) return fail(SKML_E_ARG, "w is NULL");
    if (p->kind == SKML_OPT_ADAM && (!r[1].p || !r[2].p)) return fail(SKML_E_ARG, "Adam needs m and v");
    if (p->kind == SKML_OPT_SGD && (r[1].p || r[2].p)) return fail(SKML_E_ARG, "m and v must be NULL for SGD");
    for (int i = 0; i < 3; i++)
        if (r[i].p && ((uintptr_t)r[i].p) % 16) return fail(SKML_E_ARG, "%s must be 16-byte aligned", r[i].name);
    for (int i = 0; i < nr; i++)
        for (int j = i + 1; j < nr; j++)
            if (overlap(r[i], r[j])) return fail(SKML_E_ARG, "%s and %s overlap", r[i].name, r[j].name);
    return SKML_OK;
}

// Adam.scala:54-56's loop invariants, in the reference's double arithmetic.
OptConsts consts_of(const skml_opt_params& p, int live) {
    OptConsts k{};
    k.lr = p.lr;
    k.beta1 = p.beta1;
    k.beta2 = p.beta2;
    k.omb1 = 1 - p.beta1;
    k.omb2 = 1 - p.beta2;
    k.c_m = std::sqrt(1 - p.beta2_t);
    k.c_d = 1 - p.beta1_t;
    k.eps = p.eps;
    k.live = live;
    k.adam = p.kind == SKML_OPT_ADAM;
    return k;
}

// DenseDoubleGradient.toAuto's rule (DenseDoubleGradient.scala:92-95): nnz > dim * 2 / 3 in Java
// int arithmetic (the product wraps for dim > 1,073,741,823; the division truncates toward zero).
bool auto_dense(int64_t nnz, int64_t dim) {
    const int32_t prod = (int32_t)(uint32_t)((uint64_t)dim * 2u);
    return nnz > (int64_t)(prod / 3);
}

// The live counter, zeroed on the context's stream.
int counter_zeroed(skml_ctx* c, unsigned long long** out) {
    if (const int st = reserve(c, c->opt_ws, 256, 256, "the optimiser step's live counter")) return st;
    HIP_TRY(hipMemsetAsync(c->opt_ws.p, 0, sizeof(unsigned long long), c->stream));
    *out = static_cast<unsigned long long*>(c->opt_ws.p);
    return SKML_OK;
}
// Reads the counter back (synchronises) and makes AUTO's choice: *live = 1 for LIVE.
int auto_choice(skml_ctx* c, const unsigned long long* cnt, int64_t dim, int* live) {
    unsigned long long* pin = static_cast<unsigned long long*>(ctx_pinned(c, sizeof(unsigned long long)));
    if (!pin) return fail(SKML_E_OOM, "pinned staging of the live count");
    HIP_TRY(hipMemcpyAsync(pin, cnt, sizeof(*pin), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *live = auto_dense((int64_t)*pin, dim) ? 0 : 1;
    return SKML_OK;
}

int decode_sum_step_x(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, double scale,
                      const skml_opt_params* p, int wide, void* w, void* m, void* v) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (n < 1 || n > 0x7FFFFFFFLL) return fail(SKML_E_ARG, "n=%lld outside [1, 2^31 - 1]", (long long)n);
    if (P < 1 || P > 16) return fail(SKML_E_ARG, "P=%d outside [1, 16]", P);
    const size_t sb = (size_t)n * (wide ? 8 : 4);
    Range r[4] = {{w, sb, "w"}, {m, sb, "m"}, {v, sb, "v"}, {payloads, (size_t)P * stride, "payloads"}};
    if (const int st = check_common(c, p, r, 4)) return st;
    int common_bits = 0, max_bins = 0;
    if (const int st = dense_sum_headers(c, payloads, P, stride, n, &common_bits, &max_bins)) return st;
    KernelTimer kt(c, SKML_K_DECODE_SUM);
    int live = p->select == SKML_OPT_LIVE;
    if (p->select == SKML_OPT_AUTO) {
        unsigned long long* cnt = nullptr;
        if (const int st = counter_zeroed(c, &cnt)) return st;
        HIP_TRY(launch_decode_sum_live(c->stream, payloads, P, stride, n, scale, cnt));
        if (const int st = auto_choice(c, cnt, n, &live)) return st;
    }
    HIP_TRY(launch_decode_sum_step(c->stream, payloads, P, stride, n, scale, common_bits, max_bins, consts_of(*p, live), wide,
                                   w, m, v));
    return SKML_OK;
}

// The fixed-point twin of decode_sum_step_x.  The payloads end at the last one's own bytes, which
// its header's width gives: what can be refused without the headers (a state range that reaches
// into the narrowest payloads these could be) is refused before any device work, the rest once
// fixed_sum_headers has read them back; nothing is launched before either.
int fixed_decode_sum_step_x(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, double scale,
                            const skml_opt_params* p, int wide, void* w, void* m, void* v) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (n < 1 || n > 0x7FFFFFFFLL) return fail(SKML_E_ARG, "n=%lld outside [1, 2^31 - 1]", (long long)n);
    if (P < 1 || P > 16) return fail(SKML_E_ARG, "P=%d outside [1, 16]", P);
    const size_t sb = (size_t)n * (wide ? 8 : 4), before_last = (size_t)(P - 1) * stride;
    Range r[4] = {{w, sb, "w"}, {m, sb, "m"}, {v, sb, "v"},
                  {payloads, before_last + skml_fixed_payload_bytes(n, kFxMinBits), "payloads"}};
    if (const int st = check_common(c, p, r, 4)) return st;
    int bits = 0;
    if (const int st = fixed_sum_headers(c, payloads, P, stride, n, &bits)) return st;
    r[3].bytes = before_last + skml_fixed_payload_bytes(n, bits);
    for (int i = 0; i < 3; i++)
        if (overlap(r[i], r[3])) return fail(SKML_E_ARG, "%s and %s overlap", r[i].name, r[3].name);
    KernelTimer kt(c, SKML_K_DECODE_SUM);
    int live = p->select == SKML_OPT_LIVE;
    if (p->select == SKML_OPT_AUTO) {
        unsigned long long* cnt = nullptr;
        if (const int st = counter_zeroed(c, &cnt)) return st;
        HIP_TRY(launch_fixed_decode_sum_live(c->stream, payloads, P, stride, n, scale, bits, cnt));
        if (const int st = auto_choice(c, cnt, n, &live)) return st;
    }
    HIP_TRY(launch_fixed_decode_sum_step(c->stream, payloads, P, stride, n, scale, bits, consts_of(*p, live), wide, w, m, v));
    return SKML_OK;
}

int opt_step_x(skml_ctx* c, const void* g, int32_t g_fp64, int64_t n, double scale, const skml_opt_params* p, int wide,
               void* w, void* m, void* v) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (n < 1 || n > 0x7FFFFFFFLL) return fail(SKML_E_ARG, "n=%lld outside [1, 2^31 - 1]", (long long)n);
    const size_t sb = (size_t)n * (wide ? 8 : 4);
    Range r[4] = {{w, sb, "w"}, {m, sb, "m"}, {v, sb, "v"}, {g, (size_t)n * (g_fp64 ? 8 : 4), "the gradient"}};
    if (const int st = check_common(c, p, r, 4)) return st;
    if (!g || ((uintptr_t)g) % 16) return fail(SKML_E_ARG, "the gradient must be a 16-byte aligned device pointer");
    HIP_TRY(hipSetDevice(c->device));
    KernelTimer kt(c, SKML_K_DECODE_SUM);
    int live = p->select == SKML_OPT_LIVE;
    if (p->select == SKML_OPT_AUTO) {
        unsigned long long* cnt = nullptr;
        if (const int st = counter_zeroed(c, &cnt)) return st;
        HIP_TRY(launch_opt_count(c->stream, g, g_fp64 != 0, n, scale, cnt));
        if (const int st = auto_choice(c, cnt, n, &live)) return st;
    }
    HIP_TRY(launch_opt_step(c->stream, g, g_fp64 != 0, n, scale, consts_of(*p, live), wide, w, m, v));
    return SKML_OK;
}

int opt_step_kv_x(skml_ctx* c, const int32_t* keys, const void* vals, int32_t vals_fp64, int64_t nnz, int64_t dim,
                  double scale, const skml_opt_params* p, int wide, void* w, void* m, void* v) {
    if (!c) return fail(SKML_E_ARG, "ctx is NULL");
    if (dim < 1 || dim > 0x7FFFFFFFLL || nnz < 0 || nnz > dim)
        return fail(SKML_E_ARG, "dim=%lld outside [1, 2^31 - 1] or nnz=%lld outside [0, dim]", (long long)dim, (long long)nnz);
    const size_t sb = (size_t)dim * (wide ? 8 : 4);
    Range r[5] = {{w, sb, "w"}, {m, sb, "m"}, {v, sb, "v"}, {keys, (size_t)nnz * 4, "the keys"},
                  {vals, (size_t)nnz * (vals_fp64 ? 8 : 4), "the values"}};
    if (const int st = check_common(c, p, r, 5)) return st;
    if (p->select == SKML_OPT_AUTO)
        return fail(SKML_E_ARG, "SKML_OPT_AUTO does not apply to keys and values: toAuto's choice made them");
    if (nnz > 0 && (!keys || !vals)) return fail(SKML_E_ARG, "keys or values NULL");
    HIP_TRY(hipSetDevice(c->device));
    KernelTimer kt(c, SKML_K_DECODE_SUM);
    HIP_TRY(launch_opt_step_kv(c->stream, keys, vals, vals_fp64 != 0, nnz, dim, scale,
                               consts_of(*p, p->select == SKML_OPT_LIVE), wide, w, m, v));
    return SKML_OK;
}

}  // namespace

extern "C" {

void skml_opt_params_default(skml_opt_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->kind = SKML_OPT_ADAM;
    p->select = SKML_OPT_ALL;
    p->lr = 0.0;
    p->beta1 = p->beta1_t = 0.9;
    p->beta2 = p->beta2_t = 0.999;
    p->eps = 1e-8;
}

int skml_dense_decode_sum_step_f32(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, double scale,
                                   const skml_opt_params* p, float* w, float* m, float* v) {
    return decode_sum_step_x(c, payloads, P, stride, n, scale, p, 0, w, m, v);
}

int skml_dense_decode_sum_step_f64(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, double scale,
                                   const skml_opt_params* p, double* w, double* m, double* v) {
    return decode_sum_step_x(c, payloads, P, stride, n, scale, p, 1, w, m, v);
}

int skml_fixed_decode_sum_step_f32(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, double scale,
                                   const skml_opt_params* p, float* w, float* m, float* v) {
    return fixed_decode_sum_step_x(c, payloads, P, stride, n, scale, p, 0, w, m, v);
}

int skml_fixed_decode_sum_step_f64(skml_ctx* c, const void* payloads, int32_t P, size_t stride, int64_t n, double scale,
                                   const skml_opt_params* p, double* w, double* m, double* v) {
    return fixed_decode_sum_step_x(c, payloads, P, stride, n, scale, p, 1, w, m, v);
}

int skml_opt_step_f32(skml_ctx* c, const void* g, int32_t g_fp64, int64_t n, double scale, const skml_opt_params* p,
                      float* w, float* m, float* v) {
    return opt_step_x(c, g, g_fp64, n, scale, p, 0, w, m, v);
}

int skml_opt_step_f64(skml_ctx* c, const void* g, int32_t g_fp64, int64_t n, double scale, const skml_opt_params* p,
                      double* w, double* m, double* v) {
    return opt_step_x(c, g, g_fp64, n, scale, p, 1, w, m, v);
}

int skml_opt_step_kv_f32(skml_ctx* c, const int32_t* keys, const void* vals, int32_t vals_fp64, int64_t nnz, int64_t dim,
                         double scale, const skml_opt_params* p, float* w, float* m, float* v) {
    return opt_step_kv_x(c, keys, vals, vals_fp64, nnz, dim, scale, p, 0, w, m, v);
}

int skml_opt_step_kv_f64(skml_ctx* c, const int32_t* keys, const void* vals, int32_t vals_fp64, int64_t nnz, int64_t dim,
                         double scale, const skml_opt_params* p, double* w, double* m, double* v) {
    return opt_step_kv_x(c, keys, vals, vals_fp64, nnz, dim, scale, p, 1, w, m, v);
}

}  // extern "C"
