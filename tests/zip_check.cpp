// zip_check.cpp -- host check of the ZipMLQuantizer round arithmetic (sketchml_amd/csrc/skml_zip.hpp).
// The helpers the kernels of skml_zip.hip are built from -- order-preserving keys, a pair's value
// range and error, the radix select's digit walk, the compaction's output offsets -- are driven here
// by a plain host loop shaped like the kernels (histogram per digit pass, flags + exclusive scan) and
// must give the split index list of a straightforward sequential ZipMLQuantizer.quantize
// (ml/gradient/ZipGradient.scala:70-129 with a sort-based selectKthLargest).  Built by
// tests/test_zipml_cpu.py with -fsanitize=address,undefined; prints "ok <searches>, <refusals>".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "../sketchml_amd/csrc/skml_zip.hpp"

using namespace skml;

namespace {

struct Lcg {
    uint64_t s;
    double next() {  // uniform in (-1, 1), then cubed: a peaked distribution like a gradient's
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        const double u = (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 52) - 1.0;
        return u * u * u * 1e-3;
    }
};

enum Status { kOk, kThrZero, kNoProgress };
struct Result {
    Status status;
    std::vector<int32_t> idx;
    int rounds;
};

// ---- sequential: the reference's loops ----
Result sequential(const std::vector<double>& r, const std::vector<double>& t, int64_t n, int bins) {
    std::vector<int32_t> idx(n);
    for (int64_t i = 0; i < n; i++) idx[i] = (int32_t)i;
    int64_t sn = n;
    int rounds = 0;
    while (sn > bins) {
        std::vector<double> err(sn, 0.0);
        for (int64_t i = 0; i < sn / 2; i++) {
            const int64_t L = idx[2 * i], R = (2 * i + 2 >= sn ? n : idx[2 * i + 2]) - 1;
            const double l1 = r[R] - (L == 0 ? 0 : r[L - 1]), l2 = t[R] - (L == 0 ? 0 : t[L - 1]);
            const double mean = l1 / (double)(R - L + 1);
            err[i] = l2 + mean * mean * (double)(R - L + 1) - 2 * mean * l1;
        }
        const int thr_num = bins / 2 - (sn % 2 == 1 ? 1 : 0);
        if (thr_num == 0) return {kThrZero, {}, rounds};
        std::vector<double> c(err);
        std::sort(c.begin(), c.end(), std::greater<double>());
        const double thr = c[thr_num - 1];
        int64_t m = 0;
        for (int64_t i = 0; i < sn / 2; i++) {
            idx[m++] = idx[2 * i];
            if (err[i] >= thr) idx[m++] = idx[2 * i + 1];
        }
        if (m >= sn) return {kNoProgress, {}, rounds};
        sn = m;  // an odd splitNum's last singleton is dropped
        rounds++;
    }
    idx.resize(sn);
    return {kOk, idx, rounds};
}

// ---- the kernels' shape over the shared helpers ----
Result with_helpers(const std::vector<double>& r, const std::vector<double>& t, int64_t n, int bins) {
    std::vector<int32_t> a, b(n);
    const int32_t* idx = nullptr;  // round 1: the identity
    int64_t sn = n;
    int rounds = 0;
    while (sn > bins) {
        const int64_t h = sn / 2;
        int64_t k = zip_thr_num(sn, bins);
        if (k <= 0) return {kThrZero, {}, rounds};
        std::vector<double> err(h);
        for (int64_t i = 0; i < h; i++) {
            int64_t L, R;
            zip_pair_range(idx, i, sn, n, &L, &R);
            if (L < 0 || R >= n || L > R) return {kNoProgress, {}, -1};
            err[i] = zip_pair_error(r.data(), t.data(), L, R);
        }
        uint64_t prefix = 0;
        const uint64_t zkey = zip_key64(0.0);
        for (int pass = 7; pass >= 0; pass--) {
            uint32_t hist[kZipDigits] = {};
            const int sh = kZipDigitBits * (pass + 1);
            auto match = [&](uint64_t key) { return pass == 7 || (key >> sh) == (prefix >> sh); };
            for (int64_t i = 0; i < h; i++) {
                const uint64_t key = zip_key64(err[i]);
                if (match(key)) hist[zip_digit(key, pass)]++;
            }
            if (match(zkey)) hist[zip_digit(zkey, pass)] += (uint32_t)(sn - h);
            prefix |= (uint64_t)zip_select_digit(hist, &k) << (kZipDigitBits * pass);
        }
        const double thr = zip_unkey64(prefix);
        int64_t before = 0;
        for (int64_t i = 0; i < h; i++) {
            const bool keep = err[i] >= thr;
            const int64_t pos = zip_out_pos(i, before);
            b[pos] = (int32_t)zip_split_at(idx, 2 * i);
            if (keep) b[pos + 1] = (int32_t)zip_split_at(idx, 2 * i + 1);
            before += keep;
        }
        const int64_t next = h + before;
        if (next >= sn) return {kNoProgress, {}, rounds};
        a.assign(b.begin(), b.begin() + next);
        idx = a.data();
        sn = next;
        rounds++;
    }
    std::vector<int32_t> out(sn);
    for (int64_t i = 0; i < sn; i++) out[i] = (int32_t)zip_split_at(idx, i);
    return {kOk, out, rounds};
}

bool same(const Result& x, const Result& y) { return x.status == y.status && x.idx == y.idx && x.rounds == y.rounds; }

bool prefix_of(std::vector<double> v, std::vector<double>* r, std::vector<double>* t) {
    // sort by the keys, as the device does, and check the order against operator<
    std::vector<uint64_t> keys(v.size());
    for (size_t i = 0; i < v.size(); i++) keys[i] = zip_key64(v[i]);
    std::sort(keys.begin(), keys.end());
    std::sort(v.begin(), v.end(), [](double a, double b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); });
    r->resize(v.size());
    t->resize(v.size());
    double ra = 0, ta = 0;
    for (size_t i = 0; i < v.size(); i++) {
        const double s = zip_unkey64(keys[i]);
        if (__builtin_bit_cast(uint64_t, s) != __builtin_bit_cast(uint64_t, v[i])) return false;
        (*r)[i] = i ? ra + s : s;
        (*t)[i] = i ? ta + s * s : s * s;
        ra = (*r)[i];
        ta = (*t)[i];
    }
    return true;
}

}  // namespace

int main() {
    const int64_t sizes[] = {257, 258, 300, 1000, 4097, 65539};
    const int bin_counts[] = {4, 16, 256};
    int searches = 0, refusals = 0;
    for (int64_t n : sizes)
        for (int bins : bin_counts) {
            Lcg g{(uint64_t)(n * 1000 + bins)};
            std::vector<double> v(n), r, t;
            for (auto& e : v) e = (double)(float)g.next();
            v[0] = -0.0;
            v[1] = 0.0;
            v[2] = v[3];  // a duplicate
            if (!prefix_of(v, &r, &t)) return std::printf("key order differs at n=%lld\n", (long long)n), 1;
            const Result a = sequential(r, t, n, bins), b = with_helpers(r, t, n, bins);
            if (!same(a, b) || a.status != kOk || (int)a.idx.size() > bins || (int)a.idx.size() < bins - 1)
                return std::printf("mismatch n=%lld bins=%d: status %d/%d rounds %d/%d size %zu/%zu\n", (long long)n, bins,
                                   a.status, b.status, a.rounds, b.rounds, a.idx.size(), b.idx.size()), 1;
            searches++;
        }
    {  // the two inputs on which the reference spins forever, and float keys
        std::vector<double> v(300, 0.25), r, t;
        if (!prefix_of(v, &r, &t)) return 1;
        const Result a = sequential(r, t, 300, 256), b = with_helpers(r, t, 300, 256);
        if (a.status != kNoProgress || !same(a, b)) return std::printf("all-equal: %d/%d\n", a.status, b.status), 1;
        refusals++;
        // mostly exact zeros: 2,043 of the 2,048 pairs join zeros at error 0, the 128-th largest error
        // is 0, and every pair ties with it
        Lcg g{99};
        v.assign(4097, 0.0);
        for (int i = 0; i < 4097; i += 512) v[i] = g.next();
        if (!prefix_of(v, &r, &t)) return 1;
        const Result c = sequential(r, t, 4097, 256), d = with_helpers(r, t, 4097, 256);
        if (c.status != kNoProgress || !same(c, d)) return std::printf("mostly zeros: %d/%d\n", c.status, d.status), 1;
        refusals++;
        const float fs[] = {-1.5f, -0.0f, 0.0f, 1e-45f, 3.25f};
        for (int i = 0; i < 5; i++) {
            if (zip_unkey32(zip_key32(fs[i])) != fs[i] && fs[i] == fs[i]) return 1;
            if (i && !(zip_key32(fs[i - 1]) < zip_key32(fs[i]))) return std::printf("float key order\n"), 1;
        }
        if (!zip_bad32(__builtin_inff()) || !zip_bad64(__builtin_nan("")) || zip_bad64(1.0) || zip_bad32(-0.0f)) return 1;
        if (zip_scan_depth(2048, 0) != 17 || zip_scan_depth(2049, 0) != 35 || zip_scan_depth(1 << 28, 0) != 53) return std::printf("depth\n"), 1;
    }
    std::printf("ok %d searches, %d refusals\n", searches, refusals);
    return 0;
}
