// skml_glm_dense_blocked.hpp on the host under ASan / UBSan (tests/test_glm_dense_blocked_cpu.py), for the three
// element widths: the row dot's walk (short rows and long ones, split or not) visits every element of every
// batch position exactly once and no pad; the column sum's blocks visit every row of the window once per strip,
// in batch order, the wrap included, every column is owned once, and a step the plan calls contiguous is.  The
// arrays have exactly the sizes involved, so an index outside them is the sanitizer's to report.
#include <cstdio>
#include <vector>

#include "../sketchml_amd/csrc/skml_glm_dense_blocked.hpp"

using namespace skml;

static int fail(const char* what, long a, long b, long c) {
    std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

template <int XB>
static int check(int64_t batch, int64_t dim) {
    constexpr int E = 16 / XB, V = kBlkColBytes / XB;
    BlkPlan p;
    if (!blk_plan(XB, batch, dim, &p)) return fail("no plan", XB, (long)batch, (long)dim);
    const int64_t groups = blk_row_groups(XB, dim);
    if (p.lanes < groups && p.lanes != 64) return fail("L does not cover the row", XB, (long)dim, p.lanes);
    if (p.lanes > 8 && p.lanes / 2 >= groups) return fail("L is not the smallest", XB, (long)dim, p.lanes);
    if (p.rb * p.nb < batch || (p.nb - 1) * p.rb >= batch || p.rb % kBlkU || p.rb < kBlkMinRB) return fail("blocks", XB, (long)batch, (long)dim);
    if (p.ws_bytes != (p.nb > 1 ? p.nb * dim * 8 : 0) || p.ws_bytes / XB * kBlkWsShare > batch * dim) return fail("workspace cap", XB, (long)batch, (long)dim);
    if (batch * dim > (1 << 22)) return 0;  // the plan only: the walks below hold one counter per element

    // ---- the row dot ----
    std::vector<int> seen((size_t)(batch * dim), 0);
    const int tpg = blk_teams_per_group(p);
    const int64_t teams = blk_ceil_div(blk_teams(p, batch), tpg) * tpg;  // the launch's, the last workgroup's spare teams included
    if (groups <= 64) {
        if (p.split != 1 || p.rows_in_flight != (64 / p.lanes) * kBlkRowUnroll) return fail("short plan", XB, (long)dim, p.split);
        for (int64_t tm = 0; tm < teams; tm++)
            for (int step = 0; step < kBlkShortSteps; step++)
                for (int u = 0; u < kBlkRowUnroll; u++)
                    for (int lane = 0; lane < 64; lane++) {
                        const int64_t j = blk_short_row(tm, step, u, p.lanes, lane), c = (int64_t)(lane % p.lanes) * E;
                        if (j < 0) return fail("negative position", (long)tm, u, lane);
                        for (int e = 0; e < E; e++)
                            if (j < batch && c + e < dim) seen[(size_t)(j * dim + c + e)]++;
                    }
    } else {
        if (p.lanes != 64 || p.rows_in_flight != 1 || p.split < 1 || p.split > kBlkMaxSplit || (p.split & (p.split - 1)))
            return fail("long plan", XB, (long)dim, p.split);
        if (p.split > 1 && (batch * p.split > kBlkRowTargetWaves || groups < p.split * kBlkSplitMinGroups)) return fail("split", XB, (long)batch, p.split);
        for (int64_t tm = 0; tm < teams; tm++)
            for (int s = 0; s < p.split; s++)
                for (int64_t base = 0; base < groups; base += blk_long_stride(p.split))
                    for (int q = 0; q < kBlkRowUnroll; q++)
                        for (int lane = 0; lane < 64; lane++) {
                            const int64_t c = blk_long_group(base, q, p.split, s, lane) * E;
                            for (int e = 0; e < E; e++)
                                if (tm < batch && c + e < dim) seen[(size_t)(tm * dim + c + e)]++;
                        }
    }
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) return fail("row dot: element not visited once", XB, (long)(i / dim), (long)(i % dim));

    // ---- the column sum: rows = batch + 3 with the window from the last row on, so that it wraps after one row ----
    const int64_t rows = batch + 3, pitch = blk_ceil_div(dim, E) * E, row_q = pitch / V;
    const GlmWindow win = glm_window(rows, rows - 1, batch);
    std::vector<int> xq((size_t)(rows * row_q), 0), owned((size_t)dim, 0);
    const int64_t strips = blk_strips<XB>(dim);
    if ((strips - 1) * 64 * V >= dim) return fail("a strip without a column", XB, (long)dim, (long)strips);
    for (int64_t strip = 0; strip < strips; strip++)
        for (int lane = 0; lane < 64; lane++) {
            const int64_t k0 = blk_col_of<XB>(strip, lane);
            if (k0 % V) return fail("a lane's load is misaligned", XB, (long)strip, lane);
            for (int v = 0; v < V; v++)
                if (k0 + v < dim) owned[(size_t)(k0 + v)]++;
            if (k0 >= dim) continue;
            int64_t next = 0;  // the batch positions arrive in order over the blocks
            bool wrapped = false;
            for (int64_t b = 0; b < p.nb; b++) {
                int64_t j, j1;
                blk_block_rows(p, batch, b, &j, &j1);
                if (j != next || j1 <= j) return fail("blocks out of order or empty", XB, (long)b, (long)j);
                for (; j + kBlkU <= j1; j += kBlkU) {
                    const bool cont = blk_step_contiguous(win, j);
                    for (int u = 0; u < kBlkU; u++) {
                        const int64_t r = cont ? glm_row_of(win, j) + u : glm_row_of(win, j + u);
                        if (r != (rows - 1 + j + u) % rows) return fail("a contiguous step is not", XB, (long)j, u);
                        wrapped |= r == 0 && j + u > 0;
                        xq[(size_t)(r * row_q + k0 / V)]++;
                    }
                }
                for (; j < j1; j++) {
                    const int64_t r = glm_row_of(win, j);
                    wrapped |= r == 0 && j > 0;
                    xq[(size_t)(r * row_q + k0 / V)]++;
                }
                next = j1;
            }
            if (next != batch || (batch > 1 && !wrapped)) return fail("window not walked to its end, or no wrap", XB, (long)next, (long)batch);
        }
    for (int o : owned)
        if (o != 1) return fail("column not owned once", XB, (long)dim, o);
    for (int64_t r = 0; r < rows; r++)
        for (int64_t i = 0; i < row_q; i++) {
            const bool in = (r == rows - 1 || r < batch - 1) && i * V < dim;
            if (xq[(size_t)(r * row_q + i)] != (in ? 1 : 0)) return fail("column sum: a row's word not loaded once, or a word outside", XB, (long)r, (long)i);
        }
    return 0;
}

static int check_all(int64_t batch, int64_t dim) { return check<8>(batch, dim) || check<4>(batch, dim) || check<2>(batch, dim); }

int main() {
    BlkPlan p;
    if (blk_plan(3, 1, 1, &p) || blk_plan(8, 0, 1, &p) || blk_plan(8, 1, 0, &p) || blk_plan(4, (int64_t)1 << 31, 1, &p) || blk_plan(2, 1, (int64_t)1 << 31, &p))
        return fail("a plan for bad arguments", 0, 0, 0);
    const int64_t dims[] = {1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025, 2048, 2049, 4103, 0x7FFFFFFF};
    const int64_t batches[] = {1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513, 1000, 4097, 0x7FFFFFFF};
    for (int64_t dim : dims)
        for (int64_t batch : batches)
            if (check_all(batch, dim)) return 1;
    std::printf("ok\n");
    return 0;
}
