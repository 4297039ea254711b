// valid_check.cpp -- sketchml_amd/csrc/skml_valid.hpp on the host, a program of its own built with
// -fsanitize=address,undefined (tests/test_valid_cpu.py): the index arithmetic the validation
// kernels share with this file, walked exactly as the kernels walk it, over arrays of exactly the
// lengths the kernels are given, so that a position out of range is an error here.
//   1. valid_class against the branches of ValidationUtil.scala:23-29 written out on the edge values;
//   2. the chunk walk of k_glm_seq_sum (seq_index, seq_chunk_count: stage kSeqStep values, add the
//      chunks' first `count` slots in order) against the plain forward sum, bit for bit;
//   3. the key-and-payload scatter (valid_tile, valid_step_index, valid_slot, valid_slot_offsets) as
//      eight LSD passes with digit-major tile histograms, against std::stable_sort.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../sketchml_amd/csrc/skml_valid.hpp"

using namespace skml;

static int g_bad = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL " __VA_ARGS__); \
            std::printf("\n");            \
            g_bad++;                      \
        }                                 \
    } while (0)

static uint64_t bits_of(double d) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    return b;
}

static int check_class() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct Case {
        double pre, label;
        int want;
    } cases[] = {
        {2.0, 1.0, kValidTruePos},      {-2.0, -1.0, kValidTrueNeg},   {2.0, -1.0, kValidFalsePos},
        {-2.0, 1.0, kValidFalseNeg},    {1e-200, 1e-200, kValidNone},  // the product underflows to +0.0
        {-1e-200, 1e-200, kValidNone},  {3.0, 0.0, kValidNone},        {0.0, 1.0, kValidNone},
        {-0.0, -1.0, kValidNone},       {nan, 1.0, kValidNone},        {1.0, nan, kValidNone},
        {inf, 1.0, kValidTruePos},      {-inf, 1.0, kValidFalseNeg},   {inf, 0.0, kValidNone},  // inf * 0 is NaN
        {5e-324, 1.0, kValidTruePos},   {5e-324, -0.5, kValidNone},    {0.5, 0.25, kValidTruePos},
        {-0.5, 0.25, kValidFalseNeg},   {0.5, -3.0, kValidFalsePos},   {-0.5, -3.0, kValidTrueNeg},
    };
    int n = 0;
    for (const Case& c : cases) {
        CHECK(valid_class(c.pre, c.label) == c.want, "valid_class(%g, %g) = %d, want %d", c.pre, c.label,
              valid_class(c.pre, c.label), c.want);
        n++;
    }
    return n;
}

// k_glm_seq_sum's walk with 64 lanes played one after the other.
static double seq_sum_walk(const std::vector<double>& x) {
    const int64_t n = (int64_t)x.size();
    std::vector<double> slots(kSeqStep), nxt(kSeqStep);
    auto load = [&](int64_t b) {
        for (int u = 0; u < kSeqU; u++)
            for (int lane = 0; lane < 64; lane++) {
                const int64_t i = seq_index(b, u, lane);
                nxt[u * 64 + lane] = i < n ? x.data()[i] : 0.0;
            }
    };
    double acc = 0.0;
    load(0);
    for (int64_t b = 0; b < n; b += kSeqStep) {
        slots = nxt;
        if (b + kSeqStep < n) load(b + kSeqStep);
        for (int u = 0; u < kSeqU; u++) {
            const int cnt = seq_chunk_count(n, b, u);
            CHECK(cnt >= 0 && cnt <= 64, "chunk count %d", cnt);
            for (int i = 0; i < cnt; i++) acc += slots[u * 64 + i];
        }
    }
    return acc;
}

static int check_seq_sum(std::mt19937_64& rng) {
    std::normal_distribution<double> nd;
    std::uniform_int_distribution<int> ed(-20, 20);
    const int64_t sizes[] = {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1025, 70001};
    int n = 0;
    for (int64_t sz : sizes) {
        std::vector<double> x((size_t)sz);
        for (double& v : x) v = std::ldexp(nd(rng), ed(rng));
        double fwd = 0.0;
        for (double v : x) fwd += v;
        const double got = seq_sum_walk(x);
        CHECK(bits_of(got) == bits_of(fwd), "ordered sum of %lld: %a against %a", (long long)sz, got, fwd);
        int64_t covered = 0;
        for (int64_t b = 0; b < sz; b += kSeqStep)
            for (int u = 0; u < kSeqU; u++) covered += seq_chunk_count(sz, b, u);
        CHECK(covered == sz, "the chunks of %lld cover %lld", (long long)sz, (long long)covered);
        n++;
    }
    return n;
}

// One pass as k_zip_hist + the exclusive scan + k_valid_scatter run it.
static void scatter_pass(const std::vector<uint64_t>& in, const std::vector<uint32_t>& pin, std::vector<uint64_t>& out,
                         std::vector<uint32_t>& pout, int pass) {
    const int64_t n = (int64_t)in.size();
    const int nblocks = (int)((n + kZsTile - 1) / kZsTile);
    std::vector<uint32_t> hist((size_t)kZipDigits * nblocks, 0u);
    for (int b = 0; b < nblocks; b++) {
        int64_t b0, e;
        valid_tile(b, n, &b0, &e);
        CHECK(b0 < e && e <= n, "tile %d: [%lld, %lld)", b, (long long)b0, (long long)e);
        for (int64_t i = b0; i < e; i++) hist[(size_t)zip_digit(in.data()[i], pass) * nblocks + b]++;
    }
    uint32_t run = 0;
    for (uint32_t& h : hist) {  // digit-major exclusive scan
        const uint32_t c = h;
        h = run;
        run += c;
    }
    std::vector<uint8_t> written((size_t)n, 0);
    for (int b = 0; b < nblocks; b++) {
        std::vector<uint32_t> base(kZipDigits), cnt((size_t)kValidSlots * kZipDigits, 0u), off((size_t)kValidSlots * kZipDigits, 0u);
        for (int d = 0; d < kZipDigits; d++) base[d] = hist[(size_t)d * nblocks + b];
        int64_t b0, e;
        valid_tile(b, n, &b0, &e);
        for (int64_t s0 = b0; s0 < e; s0 += kZsRows * kZsThreads) {
            std::vector<int> rank((size_t)kZsRows * kZsThreads, -1);
            for (int j = 0; j < kZsRows; j++)
                for (int wave = 0; wave < kZsWaves; wave++)
                    for (int lane = 0; lane < 64; lane++) {  // a key's rank among its wave's equal digits
                        const int tid = wave * 64 + lane;
                        const int64_t i = valid_step_index(s0, j, tid);
                        if (i >= e) continue;
                        const int d = zip_digit(in.data()[i], pass);
                        rank[(size_t)j * kZsThreads + tid] = (int)cnt[(size_t)valid_slot(j, wave) * kZipDigits + d]++;
                    }
            for (int d = 0; d < kZipDigits; d++) base[d] = valid_slot_offsets(base[d], &cnt[d], &off[d], kZipDigits);
            for (uint32_t c : cnt) CHECK(c == 0u, "a count survives the step");
            for (int j = 0; j < kZsRows; j++)
                for (int tid = 0; tid < kZsThreads; tid++) {
                    const int64_t i = valid_step_index(s0, j, tid);
                    if (i >= e) continue;
                    const int d = zip_digit(in.data()[i], pass);
                    const uint32_t pos = off[(size_t)valid_slot(j, tid / 64) * kZipDigits + d] + (uint32_t)rank[(size_t)j * kZsThreads + tid];
                    CHECK((int64_t)pos < n, "position %u of %lld", pos, (long long)n);
                    if ((int64_t)pos >= n) continue;
                    CHECK(!written[pos], "position %u written twice", pos);
                    written[pos] = 1;
                    out.data()[pos] = in.data()[i];
                    pout.data()[pos] = pin.data()[i];
                }
        }
    }
}

static int check_scatter(std::mt19937_64& rng) {
    const int64_t sizes[] = {1, 2, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 24581};
    int n = 0;
    for (int64_t sz : sizes)
        for (int form = 0; form < 3; form++) {
            std::vector<double> score((size_t)sz);
            std::normal_distribution<double> nd;
            for (int64_t i = 0; i < sz; i++) {
                if (form == 0) score[i] = nd(rng);                                  // distinct
                else if (form == 1) score[i] = (double)((int)(rng() % 5) - 2) * 0.0;  // +-0.0 only
                else score[i] = i / 1500 % 2 ? 0.25 : (double)(rng() % 7) - 3.0;     // runs of one value past a step
            }
            std::vector<uint64_t> a((size_t)sz), b((size_t)sz);
            std::vector<uint32_t> ia((size_t)sz), ib((size_t)sz);
            for (int64_t i = 0; i < sz; i++) {
                a[i] = zip_key64(score[i]);
                ia[i] = (uint32_t)i;
            }
            for (int pass = 0; pass < 8; pass++) {
                scatter_pass(a, ia, b, ib, pass);
                a.swap(b);
                ia.swap(ib);
            }
            std::vector<uint32_t> want((size_t)sz);
            for (int64_t i = 0; i < sz; i++) want[i] = (uint32_t)i;
            std::stable_sort(want.begin(), want.end(), [&](uint32_t p, uint32_t q) { return zip_key64(score[p]) < zip_key64(score[q]); });
            CHECK(ia == want, "the permutation of %lld scores, form %d", (long long)sz, form);
            for (int64_t i = 0; i < sz; i++)
                if (a[i] != zip_key64(score[ia[i]])) {
                    CHECK(false, "key %lld does not travel with its payload", (long long)i);
                    break;
                }
            n++;
        }
    return n;
}

int main() {
    std::mt19937_64 rng(20240607);
    const int c = check_class();
    const int s = check_seq_sum(rng);
    const int t = check_scatter(rng);
    if (g_bad) return 1;
    std::printf("ok %d classes %d sums %d sorts\n", c, s, t);
    return 0;
}
