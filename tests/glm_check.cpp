// glm_check.cpp -- the window split and the ordered column walk of sketchml_amd/csrc/skml_glm.hpp on
// the host, against a plain scatter in CSR order (DenseDoubleGradient.plusBy over DataSet.loopingRead),
// over random, wrapped, full and one-row windows.  A stand-alone program: built with g++ by
// tests/test_glm_cpu.py (with -fsanitize=address,undefined), it prints "ok <windows> windows".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sketchml_amd/csrc/skml_glm.hpp"

using namespace skml;

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 17;
}
// a double of either sign over about 40 binades: sums of these depend on the order
double value() {
    const double m = (double)(next() % 2000001) / 1000000.0 - 1.0;
    const int e = (int)(next() % 41) - 20;
    double s = 1.0;
    for (int i = 0; i < (e < 0 ? -e : e); i++) s *= 2.0;
    return e < 0 ? m / s : m * s;
}

struct Data {
    int64_t rows, dim;
    std::vector<int64_t> row_ptr, col_ptr;
    std::vector<int32_t> col, csc_row;
    std::vector<double> val, csc_val;
};

// rows x dim with a bias column 0 in most rows, a few hot columns and random others, columns ascending
Data make(int64_t rows, int64_t dim) {
    Data d;
    d.rows = rows;
    d.dim = dim;
    d.row_ptr.push_back(0);
    for (int64_t r = 0; r < rows; r++) {
        std::vector<char> has((size_t)dim, 0);
        if (next() % 8) has[0] = 1;
        for (int64_t h = 1; h < dim && h < 6; h++)
            if (next() % 2) has[(size_t)h] = 1;
        const int extra = (int)(next() % 4);
        for (int t = 0; t < extra; t++) has[(size_t)(next() % (uint64_t)dim)] = 1;
        if (r % 5 == 0) has[(size_t)dim - 1] = 1;
        if (r % 11 == 3) std::fill(has.begin(), has.end(), 0);  // an empty row
        for (int64_t k = 0; k < dim; k++)
            if (has[(size_t)k]) {
                d.col.push_back((int32_t)k);
                d.val.push_back(value());
            }
        d.row_ptr.push_back((int64_t)d.col.size());
    }
    // (column, row) order by counting: stable, so the rows of a column ascend
    d.col_ptr.assign((size_t)dim + 1, 0);
    for (int32_t c : d.col) d.col_ptr[(size_t)c + 1]++;
    for (int64_t k = 0; k < dim; k++) d.col_ptr[(size_t)k + 1] += d.col_ptr[(size_t)k];
    std::vector<int64_t> at(d.col_ptr.begin(), d.col_ptr.end() - 1);
    d.csc_row.resize(d.col.size());
    d.csc_val.resize(d.col.size());
    for (int64_t r = 0; r < rows; r++)
        for (int64_t i = d.row_ptr[(size_t)r]; i < d.row_ptr[(size_t)r + 1]; i++) {
            const int64_t p = at[(size_t)d.col[(size_t)i]]++;
            d.csc_row[(size_t)p] = (int32_t)r;
            d.csc_val[(size_t)p] = d.val[(size_t)i];
        }
    return d;
}

int check_window(const Data& d, int64_t row0, int64_t batch) {
    const GlmWindow w = glm_window(d.rows, row0, batch);
    std::vector<double> coef((size_t)batch);
    for (double& c : coef) c = value();
    // the reference: instance j = row (row0 + j) mod rows, its entries in stored order
    std::vector<double> want((size_t)d.dim, 0.0);
    for (int64_t j = 0; j < batch; j++) {
        const int64_t r = (row0 + j) % d.rows;
        if (glm_row_of(w, j) != r) return std::printf("row_of(%lld) of window (%lld, %lld)\n", (long long)j, (long long)row0, (long long)batch);
        for (int64_t i = d.row_ptr[(size_t)r]; i < d.row_ptr[(size_t)r + 1]; i++) {
            const double p = d.val[(size_t)i] * coef[(size_t)j];
            want[(size_t)d.col[(size_t)i]] += p;
        }
    }
    for (int64_t k = 0; k < d.dim; k++) {
        const GlmColRanges r = glm_col_ranges(d.csc_row.data(), d.col_ptr[(size_t)k], d.col_ptr[(size_t)k + 1], w);
        const double got = glm_col_sum(d.csc_row.data(), d.csc_val.data(), r, w, coef.data(), batch);
        if (std::memcmp(&got, &want[(size_t)k], 8) != 0 || r.count() < 0)
            return std::printf("column %lld of window (%lld, %lld): %a, want %a\n", (long long)k, (long long)row0,
                               (long long)batch, got, want[(size_t)k]);
    }
    return 0;
}

}  // namespace

int main() {
    int windows = 0;
    const int64_t shapes[][2] = {{1, 1}, {2, 3}, {7, 9}, {64, 40}, {130, 17}, {300, 64}};
    for (const auto& s : shapes) {
        const Data d = make(s[0], s[1]);
        std::vector<int64_t> w0 = {0, d.rows - 1, d.rows / 2}, wb = {1, d.rows, (d.rows + 1) / 2};
        for (int t = 0; t < 12; t++) {
            w0.push_back((int64_t)(next() % (uint64_t)d.rows));
            wb.push_back(1 + (int64_t)(next() % (uint64_t)d.rows));
        }
        for (int64_t row0 : w0)
            for (int64_t batch : wb) {
                if (check_window(d, row0, batch)) return 1;
                windows++;
            }
    }
    std::printf("ok %d windows\n", windows);
    return 0;
}
