// skml_glm_dense_multi.hpp on the host under ASan / UBSan (tests/test_glm_dense_multi_cpu.py), for the three element
// widths and K = 1, 2, 15, 16: the row dot's walk (R = 1 or 4 tiles per wave, split over waves or not) feeds every
// (row, column) of the window to exactly one instruction slot and no pad, and its four results per lane cover every
// (row, model) once; the column sum's strips and blocks load every word of every window row once, the wrap included,
// own every column once and store every (model, column) once per block inside the partial sums; the partial-sum cap
// holds; K x n sizes near 2^63 are refused.  The arrays have exactly the sizes involved, so an index outside them is
// the sanitizer's to report.
#include <cstdio>
#include <vector>

#include "../sketchml_amd/csrc/skml_glm_dense_multi.hpp"

using namespace skml;

static int fail(const char* what, long a, long b, long c) {
    std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

template <int XB>
static int check(int models, int64_t batch, int64_t dim) {
    constexpr int E = 16 / XB, V = 8 / XB;
    MulPlan p;
    if (!mul_plan(XB, models, batch, dim, &p)) return fail("no plan", XB, (long)batch, (long)dim);
    const int64_t tiles = mul_tiles(batch), steps = mul_col_steps(E, dim);
    if (p.lane_cols != E || p.strip_cols != 16 * kMulWords * V || (p.tiles_per_wave != 1 && p.tiles_per_wave != kMulAcc)) return fail("plan constants", XB, p.lane_cols, p.strip_cols);
    if (p.split < 1 || p.split > kMulMaxSplit || (p.split & (p.split - 1)) || (p.split > 1 && (p.tiles_per_wave != 1 || tiles * p.split > kMulRowTargetWaves || steps < mul_step_stride(p))))
        return fail("split", XB, (long)batch, p.split);
    if (p.rb * p.nb < batch || (p.nb - 1) * p.rb >= batch || p.rb % kMulRowsPerIter || p.rb < mul_min_rb(XB, models)) return fail("blocks", XB, (long)batch, (long)dim);
    if (p.ws_bytes != (p.nb > 1 ? p.nb * models * dim * 8 : 0) || p.ws_bytes / XB * kMulWsShare > batch * dim) return fail("workspace cap", XB, (long)batch, (long)dim);
    if (batch * dim > (1 << 22)) return 0;  // the plan only: the walks below hold one counter per element

    // ---- the row dot: the x operand's (row, column) per instruction slot, then the results' (row, model) ----
    std::vector<int> seen((size_t)(batch * dim), 0), outs((size_t)(batch * models), 0);
    const int tpg = mul_teams_per_group(p), R = p.tiles_per_wave;
    const int64_t teams = mul_ceil_div(mul_teams(p, batch), tpg) * tpg;  // the launch's, the last workgroup's spare teams included
    for (int64_t tm = 0; tm < teams; tm++)
        for (int r = 0; r < R; r++) {
            const int64_t tile = tm * R + r;
            for (int s = 0; s < p.split; s++)
                for (int64_t base = 0; base < steps; base += mul_step_stride(p))
                    for (int a = 0; a < mul_steps_in_flight(R); a++) {
                        const int64_t step = mul_step_of(base, a, p.split, s);
                        if (step >= steps) continue;  // mode 0 of the kernel
                        for (int lane = 0; lane < 64; lane++) {
                            const int64_t j = tile * kMulTileRows + lane % 16, c = mul_lane_col(step, lane / 16, E);
                            if (c % E) return fail("a lane's load is misaligned", XB, (long)step, lane);
                            for (int e = 0; e < E; e++)
                                if (tile < tiles && j < batch && c + e < dim) seen[(size_t)(j * dim + c + e)]++;
                        }
                    }
            for (int lane = 0; lane < 64; lane++)
                for (int rr = 0; rr < 4; rr++) {
                    const int64_t j = mul_out_row(tile, lane, rr);
                    if (tile < tiles && lane % 16 < models && j < batch) outs[(size_t)((lane % 16) * batch + j)]++;
                }
        }
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) return fail("row dot: element not fed once", XB, (long)(i / dim), (long)(i % dim));
    for (size_t i = 0; i < outs.size(); i++)
        if (outs[i] != 1) return fail("row dot: result not stored once", XB, (long)(i / batch), (long)(i % batch));

    // ---- the column sum: rows = batch + 3 with the window from the last row on, so that it wraps after one row ----
    const int64_t rows = batch + 3, pitch = mul_ceil_div(dim, E) * E, row_q = pitch / V;
    const GlmWindow win = glm_window(rows, rows - 1, batch);
    std::vector<int> xq((size_t)(rows * row_q), 0), owned((size_t)dim, 0), coef((size_t)(models * batch), 0);
    std::vector<int> part((size_t)(p.nb * models * dim), 0);
    const int64_t strips = mul_strips(XB, dim);
    if (mul_col_of<XB>(strips - 1, 0, 0) >= dim) return fail("a strip without a column", XB, (long)dim, (long)strips);
    for (int64_t strip = 0; strip < mul_ceil_div(strips, kMulColWaves) * kMulColWaves; strip++) {
        if (mul_col_of<XB>(strip, 0, 0) >= dim) continue;  // the kernel's wave-uniform test
        for (int64_t b = 0; b < p.nb; b++) {
            int64_t j0, j1;
            mul_block_rows(p, batch, b, &j0, &j1);
            if (j0 != b * p.rb || j1 <= j0 || j1 > batch || (b == p.nb - 1 && j1 != batch)) return fail("blocks out of order or empty", XB, (long)b, (long)j0);
            for (int lane = 0; lane < 64; lane++) {
                const int n = lane % 16, k = lane / 16;
                for (int64_t j = j0; j < j1; j += kMulRowsPerIter)
                    for (int u = 0; u < kMulU; u++) {
                        const int64_t jj = mul_row_pos(j, u, k);
                        if (jj >= j1) continue;
                        const int64_t row = glm_row_of(win, jj);
                        if (row != (rows - 1 + jj) % rows) return fail("a window row is not", XB, (long)jj, (long)row);
                        for (int t = 0; t < kMulWords; t++) {
                            const int64_t c0 = mul_col_of<XB>(strip, t, n);
                            if (c0 % V) return fail("a lane's word is misaligned", XB, (long)strip, lane);
                            if (c0 < dim) xq[(size_t)(row * row_q + c0 / V)]++;
                        }
                        if (strip == 0 && n < models) coef[(size_t)(n * batch + jj)]++;
                    }
                for (int r = 0; r < 4; r++) {
                    const int m = mul_out_model(lane, r);
                    if (m >= models) continue;
                    for (int t = 0; t < kMulWords; t++)
                        for (int v = 0; v < V; v++) {
                            const int64_t c = mul_col_of<XB>(strip, t, n) + v;
                            if (c >= dim) continue;
                            part[(size_t)((b * models + m) * dim + c)]++;
                            if (b == 0 && m == 0) owned[(size_t)c]++;
                        }
                }
            }
        }
    }
    for (int o : owned)
        if (o != 1) return fail("column not owned once", XB, (long)dim, o);
    for (int o : part)
        if (o != 1) return fail("a partial sum not stored once", XB, (long)dim, o);
    for (int o : coef)
        if (o != 1) return fail("a coef not loaded once by a strip", XB, (long)batch, o);
    for (int64_t r = 0; r < rows; r++)
        for (int64_t i = 0; i < row_q; i++) {
            const bool in = (r == rows - 1 || r < batch - 1) && i * V < dim;
            if (xq[(size_t)(r * row_q + i)] != (in ? 1 : 0)) return fail("column sum: a row's word not loaded once, or a word outside", XB, (long)r, (long)i);
        }
    return 0;
}

static int check_all(int models, int64_t batch, int64_t dim) { return check<8>(models, batch, dim) || check<4>(models, batch, dim) || check<2>(models, batch, dim); }

int main() {
    MulPlan p;
    if (mul_plan(3, 1, 1, 1, &p) || mul_plan(8, 0, 1, 1, &p) || mul_plan(8, 17, 1, 1, &p) || mul_plan(8, 1, 0, 1, &p) || mul_plan(8, 1, 1, 0, &p) ||
        mul_plan(4, 1, (int64_t)1 << 31, 1, &p) || mul_plan(2, 1, 1, (int64_t)1 << 31, &p))
        return fail("a plan for bad arguments", 0, 0, 0);
    int64_t bytes = 0;
    const int64_t top = INT64_MAX / 8;
    if (!mul_bytes(16, top / 16, &bytes) || bytes != top / 16 * 16 * 8 || !mul_bytes(1, top, &bytes) || !mul_bytes(0, top, &bytes) || bytes != 0)
        return fail("a size that fits is refused", 0, 0, 0);
    if (mul_bytes(16, top / 16 + 1, &bytes) || mul_bytes(2, top, &bytes) || mul_bytes(16, INT64_MAX, &bytes) || mul_bytes(1, top + 1, &bytes) ||
        mul_bytes(-1, 1, &bytes) || mul_bytes(1, -1, &bytes))
        return fail("a size beyond an int64 is not refused", 0, 0, 0);
    const int64_t dims[] = {1, 2, 3, 4, 5, 7, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 257, 513, 1025, 2049, 4103, 0x7FFFFFFF};
    const int64_t batches[] = {1, 2, 15, 16, 17, 63, 65, 255, 256, 257, 513, 1000, 1025, 4097, 0x7FFFFFFF};
    const int ks[] = {1, 2, 15, 16};
    for (int k : ks)
        for (int64_t dim : dims)
            for (int64_t batch : batches)
                if (check_all(k, batch, dim)) return 1;
    // enough tiles for R = 4, ending inside a tile; a long row of few rows, split over waves
    if (check_all(2, 65536 + 5, 5) || check_all(16, 65536, 3) || check_all(15, 3, 4 * 8 * 9 + 3) || check_all(2, 18, 4 * 8 * 64)) return 1;
    if (!mul_plan(8, 2, 65541, 5, &p) || p.tiles_per_wave != kMulAcc || !mul_plan(2, 15, 3, 291, &p) || p.split < 2) return fail("the sweep misses R = 4 or S > 1", 0, 0, 0);
    std::printf("ok\n");
    return 0;
}
