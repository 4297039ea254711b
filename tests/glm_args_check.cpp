// skml_glm_args.hpp on the host under ASan / UBSan (tests/test_glm_args_cpu.py): a table of cases over the argument
// checks of the mini-batch gradient and validation entries, each with the status and the word of the message that the
// entries had when every family carried its own copy of the checks.  The ranges are integers cast to pointers; nothing
// is dereferenced.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../sketchml_amd/csrc/skml_glm_args.hpp"

using namespace skml;

static int g_code = 0;
static char g_msg[512] = "";
int skml::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    g_code = code;
    return code;
}

static int g_bad = 0;
// st is what the check returned; `word`, and `word2` when given, must be in the message of a refusal.
static void expect(const char* what, int st, int want, const char* word = nullptr, const char* word2 = nullptr) {
    bool ok = st == want;
    if (ok && want != SKML_OK) ok = g_code == want && (!word || std::strstr(g_msg, word)) && (!word2 || std::strstr(g_msg, word2));
    if (!ok) {
        std::printf("FAIL %s: status %d (wanted %d), message \"%s\" (wanted \"%s\" \"%s\")\n", what, st, want, st ? g_msg : "", word ? word : "",
                    word2 ? word2 : "");
        g_bad++;
    }
}
static const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }
static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// ---- the range checker: two in, three out, grad; ids 0 .. 5 in that order ----
struct Set {
    Range r[6] = {{at(0x1000), 64, "label"}, {at(0x2000), 64, "w"}, {at(0x3000), 64, "pre_out"},
                  {at(0x4000), 64, "coef_out"}, {at(0x5000), 64, "loss_out"}, {at(0x6000), 128, "grad_out"}};
    int check() const { return ranges_check(r, 2, r + 2, 3, &r[5]); }
};

static void range_cases() {
    expect("the base set", Set().check(), SKML_OK);
    for (int i = 0; i < 6; i++) {
        Set s;
        s.r[i].p = at(addr(s.r[i].p) + 4);
        expect("off by 4", s.check(), SKML_E_ARG, s.r[i].name, "8-byte aligned");
    }
    {  // two inputs may share memory
        Set s;
        s.r[1].p = s.r[0].p;
        expect("in on in", s.check(), SKML_OK);
    }
    // (written x, other y): grad against in, grad against out, each out against each in, out against out
    const int pairs[][2] = {{5, 0}, {5, 1}, {5, 2}, {5, 3}, {5, 4}, {2, 0}, {2, 1}, {3, 0}, {3, 1}, {4, 0}, {4, 1}, {2, 3}, {2, 4}, {3, 4}};
    for (const auto& pr : pairs) {
        const int x = pr[0], y = pr[1];
        Set s;
        // x begins inside y's last byte; then where y ends
        s.r[y].bytes = 57;
        s.r[x].p = at(addr(s.r[y].p) + 56);
        expect("one byte at y's end", s.check(), SKML_E_ARG, s.r[x].name, s.r[y].name);
        s.r[y].bytes = 56;
        expect("touching y's end", s.check(), SKML_OK);
        // x's last byte is y's first; then x ends where y begins
        s = Set();
        s.r[x].p = at(addr(s.r[y].p) - 56);
        s.r[x].bytes = 57;
        expect("one byte at y's start", s.check(), SKML_E_ARG, s.r[x].name, s.r[y].name);
        s.r[x].bytes = 56;
        expect("touching y's start", s.check(), SKML_OK);
        // a NULL or an empty range overlaps nothing
        s = Set();
        s.r[x] = {nullptr, SIZE_MAX, s.r[x].name};
        expect("x NULL", s.check(), SKML_OK);
        s = Set();
        s.r[x] = {s.r[y].p, 0, s.r[x].name};
        expect("x empty", s.check(), SKML_OK);
        s = Set();
        s.r[y] = {s.r[x].p, 0, s.r[y].name};
        expect("y empty", s.check(), SKML_OK);
    }
    {  // two faults: every alignment before any overlap, in then out then grad
        Set s;
        s.r[2].p = s.r[0].p;
        s.r[5].p = at(addr(s.r[5].p) + 4);
        expect("pre on label, grad off by 4", s.check(), SKML_E_ARG, "grad_out", "aligned");
        s = Set();
        s.r[4].p = at(addr(s.r[4].p) + 4);
        s.r[1].p = at(addr(s.r[1].p) + 4);
        expect("loss and w off by 4", s.check(), SKML_E_ARG, "w must");
    }
    {  // grad against in, then grad against out before that out against in, out against out last
        Set s;
        s.r[2].p = s.r[0].p;
        s.r[5].p = s.r[1].p;
        expect("pre on label, grad on w", s.check(), SKML_E_ARG, "grad_out", "w");
        s = Set();
        s.r[2].p = s.r[0].p;
        s.r[5].p = s.r[4].p;
        expect("pre on label, grad on loss", s.check(), SKML_E_ARG, "pre_out", "label");
        s = Set();
        s.r[3].p = s.r[0].p;
        s.r[5].p = s.r[2].p;
        expect("coef on label, grad on pre", s.check(), SKML_E_ARG, "grad_out", "pre_out");
        s = Set();
        s.r[2].p = s.r[3].p;
        s.r[4].p = s.r[1].p;
        expect("pre on coef, loss on w", s.check(), SKML_E_ARG, "loss_out", "w");
    }
    // the validate form: no grad, two outs, pre_out NULL
    Range in[] = {{at(0x1000), 64, "label"}, {at(0x2000), 64, "w"}};
    Range out[] = {{nullptr, 64, "pre_out"}, {at(0x5000), 64, "loss_out"}};
    expect("validate, pre NULL", ranges_check(in, 2, out, 2, nullptr), SKML_OK);
    out[1].p = at(0x2038);
    expect("validate, loss on w", ranges_check(in, 2, out, 2, nullptr), SKML_E_ARG, "loss_out", "w");
    out[1].p = at(0x5004);
    expect("validate, loss off by 4", ranges_check(in, 2, out, 2, nullptr), SKML_E_ARG, "loss_out", "aligned");
    out[0].p = at(0x5000);
    out[1].p = at(0x5038);
    expect("validate, pre on loss", ranges_check(in, 2, out, 2, nullptr), SKML_E_ARG, "pre_out", "loss_out");
    out[1].p = at(0x5040);
    expect("validate, pre touches loss", ranges_check(in, 2, out, 2, nullptr), SKML_OK);
    in[0].p = at(0x1004);
    out[1].p = at(0x5038);
    expect("validate, label off by 4 and pre on loss", ranges_check(in, 2, out, 2, nullptr), SKML_E_ARG, "label", "aligned");
}

static void window_and_loss_cases() {
    const int64_t rows = 10;
    expect("row0 -1", window_check(rows, -1, 1), SKML_E_ARG, "row0=-1");
    expect("row0 rows - 1", window_check(rows, rows - 1, rows), SKML_OK);
    expect("row0 rows", window_check(rows, rows, 1), SKML_E_ARG, "row0=10");
    expect("batch 0", window_check(rows, 0, 0), SKML_E_ARG, "batch=0", "wraps at most once");
    expect("batch rows", window_check(rows, 3, rows), SKML_OK);
    expect("batch rows + 1", window_check(rows, 3, rows + 1), SKML_E_ARG, "batch=11", "wraps at most once");
    expect("row0 and batch", window_check(rows, rows, 0), SKML_E_ARG, "row0=10");
    const int losses[] = {SKML_LOSS_L1_LOG, SKML_LOSS_L2_HINGE, SKML_LOSS_L2_LOG, SKML_LOSS_L2_SQUARE};
    for (int l : losses) expect("a loss", loss_check(l), SKML_OK);
    expect("loss -1", loss_check(-1), SKML_E_ARG, "unknown loss -1");
    expect("loss 4", loss_check(4), SKML_E_ARG, "unknown loss 4");
}

static void struct_cases() {
    const int64_t big = (int64_t)1 << 31;
    size_t bytes = 0;
    skml_glm_data sp = {};
    sp.rows = 3, sp.dim = 5;
    expect("sparse", sparse_check(&sp), SKML_OK);
    sp.nnz = -1;
    expect("sparse, nnz -1", sparse_check(&sp), SKML_E_ARG, "nnz=-1");
    sp.nnz = 0, sp.rows = big;
    expect("sparse, rows 2^31", sparse_check(&sp), SKML_E_ARG, "outside [1, 2^31 - 1]");

    const int64_t heads[][2] = {{0, 5}, {3, 0}, {big, 5}, {3, big}, {-1, 5}};
    for (const auto& h : heads) {
        const skml_glm_dense_data d = {h[0], h[1], nullptr, nullptr};
        expect("dense head", dense_check(&d, &bytes), SKML_E_ARG, "outside [1, 2^31 - 1]");
        const skml_glm_dense_lowp_data l = {h[0], h[1], 8, nullptr, nullptr, SKML_X_F32};
        expect("lowp head", dense_lowp_check(&l, &bytes), SKML_E_ARG, "outside [1, 2^31 - 1]");
    }
    skml_glm_dense_data d = {3, 5, nullptr, nullptr};
    expect("dense", dense_check(&d, &bytes), SKML_OK);
    if (bytes != 3 * 5 * 8) expect("dense bytes", SKML_E_ARG, SKML_OK);
    d = {big - 1, big - 1, nullptr, nullptr};  // (2^31 - 1)^2 fits an int64, times 8 does not
    expect("dense, rows * dim * 8 beyond an int64", dense_check(&d, &bytes), SKML_E_ARG, "do not fit an int64");
    d = {big - 1, (int64_t)1 << 29, nullptr, nullptr};  // just below 2^63
    expect("dense, the largest that fits", dense_check(&d, &bytes), SKML_OK);
    if (bytes != (size_t)(big - 1) << 32) expect("dense bytes near 2^63", SKML_E_ARG, SKML_OK);

    skml_glm_dense_lowp_data l = {3, 5, 8, at(0x1000), nullptr, SKML_X_F32};
    expect("lowp f32", dense_lowp_check(&l, &bytes), SKML_OK);
    if (bytes != 3 * 8 * 4) expect("lowp f32 bytes", SKML_E_ARG, SKML_OK);
    l.x_kind = SKML_X_BF16;
    expect("lowp bf16", dense_lowp_check(&l, &bytes), SKML_OK);
    if (bytes != 3 * 8 * 2) expect("lowp bf16 bytes", SKML_E_ARG, SKML_OK);
    l.x_kind = 3;
    expect("lowp, unknown kind", dense_lowp_check(&l, &bytes), SKML_E_ARG, "unknown x_kind 3");
    l.x_kind = -1;
    expect("lowp, kind -1", dense_lowp_check(&l, &bytes), SKML_E_ARG, "unknown x_kind -1");
    l = {3, 5, 4, at(0x1000), nullptr, SKML_X_F32};
    expect("lowp, pitch below dim", dense_lowp_check(&l, &bytes), SKML_E_ARG, "pitch=4");
    l.pitch = 6;
    expect("lowp f32, pitch off 4 elements", dense_lowp_check(&l, &bytes), SKML_E_ARG, "pitch=6");
    l.pitch = 12, l.x_kind = SKML_X_F16;
    expect("lowp f16, pitch off 8 elements", dense_lowp_check(&l, &bytes), SKML_E_ARG, "pitch=12");
    l.pitch = 16, l.x = at(0x1008);
    expect("lowp, x off 16 bytes", dense_lowp_check(&l, &bytes), SKML_E_ARG, "16-byte aligned");
    l = {3, 5, 4, at(0x1008), nullptr, 7};
    expect("lowp, kind before pitch before x", dense_lowp_check(&l, &bytes), SKML_E_ARG, "x_kind");
    l = {big - 1, big - 1, (int64_t)1 << 62, at(0x1000), nullptr, SKML_X_F32};
    expect("lowp, rows * pitch beyond an int64", dense_lowp_check(&l, &bytes), SKML_E_ARG, "do not fit an int64");
    l = {big - 1, big - 1, (int64_t)1 << 31, at(0x1000), nullptr, SKML_X_F32};  // 2^62 elements of 4 bytes
    expect("lowp, rows * pitch * 4 beyond an int64", dense_lowp_check(&l, &bytes), SKML_E_ARG, "do not fit an int64");
}

// ---- the dense gradient's check: rows 100, dim 40, window of 30; every array apart ----
struct Dense {
    int64_t rows = 100, dim = 40, row0 = 90, batch = 30;
    int32_t loss = SKML_LOSS_L2_LOG, models = 1;
    int wide = 1;
    uintptr_t x = 0x100000, label = 0x200000, w = 0x300000, labels = 0, pre = 0x500000, coef = 0x600000, lossj = 0x700000, grad = 0x800000;
    uintptr_t nnz = 0x900000, obj = 0x900100;
    int check() const {
        const GlmOut o = {(double*)at(pre), (double*)at(coef), (double*)at(lossj), (double*)at(grad), (int64_t*)at(nnz), (double*)at(obj)};
        return dense_gradient_check(rows, dim, at(x), (size_t)rows * dim * 8, (const double*)at(label), row0, batch, loss, models, at(w), wide,
                                    (const double*)at(labels), o);
    }
};

static void dense_gradient_cases() {
    expect("one model", Dense().check(), SKML_OK);
    Dense d;
    d.models = 0;
    expect("models 0", d.check(), SKML_E_ARG, "models=0");
    d.models = 17;
    expect("models 17", d.check(), SKML_E_ARG, "models=17");
    // the order: window, loss, models, sizes, NULLs, ranges
    d = Dense();
    d.row0 = -1, d.loss = 9;
    expect("row0 before loss", d.check(), SKML_E_ARG, "row0");
    d = Dense();
    d.loss = 9, d.models = 0;
    expect("loss before models", d.check(), SKML_E_ARG, "unknown loss 9");
    d = Dense();
    d.models = 17, d.x = 0;
    expect("models before NULL", d.check(), SKML_E_ARG, "models=17");
    d = Dense();
    d.x = 0, d.w += 4;
    expect("NULL before alignment", d.check(), SKML_E_ARG, "is NULL");
    d = Dense();
    d.grad = 0;
    expect("grad NULL", d.check(), SKML_E_ARG, "grad_out is NULL");
    d = Dense();
    d.obj = 0;
    expect("obj_loss_out NULL", d.check(), SKML_E_ARG, "obj_loss_out is NULL");
    d = Dense();
    d.pre = d.coef = d.lossj = 0;
    expect("pre, coef, loss NULL", d.check(), SKML_OK);
    d = Dense();
    d.labels = d.label + 4;
    d.models = 2;
    expect("labels off by 4", d.check(), SKML_E_ARG, "labels", "aligned");

    // K = 16: w is 16 * dim * 8 bytes of doubles and 16 * dim * 4 of floats, labels 16 * rows * 8, an out 16 * batch * 8
    for (int wide = 0; wide < 2; wide++) {
        d = Dense();
        d.models = 16, d.wide = wide, d.labels = 0x400000;
        expect("16 models", d.check(), SKML_OK);
        const uintptr_t wb = (uintptr_t)16 * 40 * (wide ? 8 : 4);
        d.grad = d.w + wb;
        expect("grad where w ends", d.check(), SKML_OK);
        d.grad = d.w + wb - 8;
        expect("grad on w's last word", d.check(), SKML_E_ARG, "grad_out", "w");
        d.grad = d.w - 16 * 40 * 8;
        expect("grad ends where w begins", d.check(), SKML_OK);
        d.grad += 8;
        expect("grad's last word on w", d.check(), SKML_E_ARG, "grad_out", "w");
    }
    d = Dense();
    d.models = 16, d.labels = 0x400000;
    d.grad = d.labels + 16 * 100 * 8;
    expect("grad where labels ends", d.check(), SKML_OK);
    d.grad -= 8;
    expect("grad on labels' last word", d.check(), SKML_E_ARG, "grad_out", "labels");
    d.grad = 0x800000, d.coef = d.pre + 16 * 30 * 8;
    expect("coef where pre ends", d.check(), SKML_OK);
    d.coef -= 8;
    expect("coef on pre's last word", d.check(), SKML_E_ARG, "pre_out", "coef_out");
    d.models = 15;  // the same addresses with one model fewer are apart
    expect("15 models", d.check(), SKML_OK);
    d = Dense();  // one model: an out is batch * 8 bytes
    d.coef = d.pre + 30 * 8;
    expect("one model, coef where pre ends", d.check(), SKML_OK);

    // K x n doubles beyond an int64: the struct's check is not this function's, so rows may be anything here
    d = Dense();
    d.rows = d.batch = INT64_MAX / 8, d.row0 = 0, d.models = 16;
    expect("16 * batch * 8 beyond an int64", d.check(), SKML_E_ARG, "do not fit an int64");
    int64_t b = 0;
    if (mul_bytes(16, INT64_MAX / 8 / 16 + 1, &b) || !mul_bytes(16, INT64_MAX / 8 / 16, &b)) expect("mul_bytes at the edge", SKML_E_ARG, SKML_OK);
}

int main() {
    range_cases();
    window_and_loss_cases();
    struct_cases();
    dense_gradient_cases();
    if (g_bad) return 1;
    std::printf("ok\n");
    return 0;
}
