// skml_glm_dense_blocked.hpp -- the plan and the index arithmetic of the dense mini-batch gradient in the
// blocked summation order (skml_glm_dense_blocked.hip): how many lanes share a row of the row dot, how many
// waves a long row is split over, which 16-byte group of a row a lane loads at which step, and how the
// window's rows are cut into the blocks of the column sum.  Everything is a function of the storage width
// (8, 4 or 2 bytes), batch and dim and of the constants below, never of the device: that is what makes the
// order of every sum, and so its bits, the same on every run.  No device builtins: the kernels and the host
// program tests/glm_dense_blocked_check.cpp instantiate the same functions.
#pragma once
#include <stdint.h>

#include "skml_glm.hpp"

namespace skml {

// ---- the row dot: L lanes share a row, each runs a chain over its own 16-byte groups ----
constexpr int kBlkRowUnroll = 4;           // loads a lane keeps in flight: rows of a short row, segments of a long one
constexpr int kBlkTeamWaves = 4;           // waves of a workgroup when a row is not split
constexpr int kBlkMaxSplit = 8;            // waves one row is split over at the most
constexpr int kBlkShortSteps = 4;           // steps of kBlkRowUnroll row sets a wave makes with one load of its group of w
constexpr int64_t kBlkRowTargetWaves = 4096;  // a row is split while batch * S stays at or below this: 4 waves per SIMD of 1,024
constexpr int64_t kBlkSplitMinGroups = 64 * kBlkRowUnroll;  // ... and every wave keeps one full unrolled step

// The column sum: a lane owns the columns of one 8-byte load, which every storage type can make on an
// 8-byte boundary whatever dim is (a double row is only 8-byte aligned when dim is odd).
constexpr int kBlkColBytes = 8;
constexpr int kBlkU = 16;                     // rows of loads in flight ahead of the dependent FMAs
constexpr int64_t kBlkMinRB = 256;            // floor of the rows of a block, a multiple of kBlkU
constexpr int64_t kBlkColTargetWaves = 4096;  // strips * NB aims at 4 waves per SIMD
constexpr int kBlkColWaves = 4;               // waves (strips) of a workgroup of the column sum
static_assert(kBlkMinRB % kBlkU == 0, "only the window's last block has a partial step");

// Elements of one 16-byte group; 0 for a width that is no storage type.
SKML_GLM_HD int blk_elems_per_group(int x_bytes) { return x_bytes == 8 || x_bytes == 4 || x_bytes == 2 ? 16 / x_bytes : 0; }
SKML_GLM_HD int64_t blk_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// 16-byte groups that cover a row of dim elements.
SKML_GLM_HD int64_t blk_row_groups(int x_bytes, int64_t dim) { return blk_ceil_div(dim, blk_elems_per_group(x_bytes)); }

struct BlkPlan {
    int lanes;           // L: lanes that share a row, 8, 16, 32 or 64
    int split;           // S: waves that share a row, 1, 2, 4 or 8 (above 1 only for a row of more than 64 groups)
    int rows_in_flight;  // rows one wave (one team of S waves) has loads in flight of
    int64_t rb, nb;      // the column sum: rows per block, blocks
    int64_t ws_bytes;    // nb * dim doubles of partial sums, 0 when nb == 1
};

// The smallest L of 8, 16, 32, 64 whose 16-byte loads cover the row; 64 for every longer row.
SKML_GLM_HD int blk_lanes(int64_t groups) { return groups <= 8 ? 8 : groups <= 16 ? 16 : groups <= 32 ? 32 : 64; }
// Waves a row is split over.
SKML_GLM_HD int blk_split(int64_t groups, int64_t batch) {
    int s = 1;
    while (s < kBlkMaxSplit && batch * (2 * s) <= kBlkRowTargetWaves && groups >= 2 * s * kBlkSplitMinGroups) s *= 2;
    return s;
}
// Rows per block of the column sum: the share of a block when the strips alone are too few waves, never
// below the floor, a multiple of kBlkU.  With nb >= 2 blocks batch > rb >= kBlkMinRB, so nb < 2 * batch / kBlkMinRB
// and the partial sums hold fewer than batch * dim * 16 / kBlkMinRB bytes: at most 1 / 32 of the window's
// bytes of x for the narrowest type (kBlkWsShare).
constexpr int64_t kBlkWsShare = 32;
template <int XB>
SKML_GLM_HD int64_t blk_strips(int64_t dim) { return blk_ceil_div(dim, 64 * (kBlkColBytes / XB)); }
SKML_GLM_HD int64_t blk_rows_per_block(int64_t strips, int64_t batch) {
    const int64_t nb0 = blk_ceil_div(kBlkColTargetWaves, strips);
    const int64_t rb = blk_ceil_div(blk_ceil_div(batch, nb0), kBlkU) * kBlkU;
    return rb < kBlkMinRB ? kBlkMinRB : rb;
}

// The plan of one call; false for a bad argument.
SKML_GLM_HD bool blk_plan(int x_bytes, int64_t batch, int64_t dim, BlkPlan* p) {
    if (!blk_elems_per_group(x_bytes) || batch < 1 || dim < 1 || batch > 0x7FFFFFFFLL || dim > 0x7FFFFFFFLL) return false;
    const int64_t groups = blk_row_groups(x_bytes, dim);
    p->lanes = blk_lanes(groups);
    p->split = groups > 64 ? blk_split(groups, batch) : 1;
    p->rows_in_flight = groups > 64 ? 1 : (64 / p->lanes) * kBlkRowUnroll;
    const int64_t strips = x_bytes == 8 ? blk_strips<8>(dim) : x_bytes == 4 ? blk_strips<4>(dim) : blk_strips<2>(dim);
    p->rb = blk_rows_per_block(strips, batch);
    p->nb = blk_ceil_div(batch, p->rb);
    p->ws_bytes = p->nb > 1 ? p->nb * dim * 8 : 0;
    return true;
}

// ---- the row dot's walk ----
// Short rows (at most 64 groups): a team is one wave, lane = sub * L + gl; at slot u (0 .. kBlkRowUnroll) of step
// `step` (0 .. kBlkShortSteps) of team tm the lane works on batch position blk_short_row(...) and on group gl of
// that row, its only one.
SKML_GLM_HD int64_t blk_short_rows_per_team(int lanes) { return (int64_t)(64 / lanes) * kBlkRowUnroll * kBlkShortSteps; }
SKML_GLM_HD int64_t blk_short_row(int64_t tm, int step, int u, int lanes, int lane) {
    return ((tm * kBlkShortSteps + step) * kBlkRowUnroll + u) * (64 / lanes) + lane / lanes;
}
// Long rows (more than 64 groups, L = 64): team tm is the S waves of batch position tm.  Wave s, lane `lane` takes at slot q
// (0 .. kBlkRowUnroll) of the step that starts at group `base` the group below; a step covers 64 * S * kBlkRowUnroll
// groups and the steps start at 0, stride, 2 * stride ... below the row's group count.
SKML_GLM_HD int64_t blk_long_stride(int split) { return (int64_t)64 * split * kBlkRowUnroll; }
SKML_GLM_HD int64_t blk_long_group(int64_t base, int q, int split, int s, int lane) { return base + ((int64_t)q * split + s) * 64 + lane; }
// Teams of the launch and the teams of one workgroup (kBlkTeamWaves waves, or the S waves of one row).
SKML_GLM_HD int64_t blk_teams(const BlkPlan& p, int64_t batch) {
    return p.rows_in_flight == 1 ? batch : blk_ceil_div(batch, blk_short_rows_per_team(p.lanes));
}
SKML_GLM_HD int blk_teams_per_group(const BlkPlan& p) { return p.split > 1 ? 1 : kBlkTeamWaves; }

// ---- the column sum's walk ----
// First column of `lane` of strip `strip`: a lane owns V = kBlkColBytes / XB adjacent columns, a wave's load of a
// row reads 512 contiguous bytes.
template <int XB>
SKML_GLM_HD int64_t blk_col_of(int64_t strip, int lane) { return (strip * 64 + lane) * (kBlkColBytes / XB); }
// Batch positions [*j0, *j1) of block b.
SKML_GLM_HD void blk_block_rows(const BlkPlan& p, int64_t batch, int64_t b, int64_t* j0, int64_t* j1) {
    *j0 = b * p.rb;
    *j1 = *j0 + p.rb < batch ? *j0 + p.rb : batch;
}
// Whether the kBlkU batch positions from j on are consecutive rows of x, so that a row's address is the one
// before plus the pitch; a step that holds the window's wrap takes glm_row_of per row instead.
SKML_GLM_HD bool blk_step_contiguous(const GlmWindow& w, int64_t j) { return glm_row_of(w, j + kBlkU - 1) == glm_row_of(w, j) + kBlkU - 1; }

}  // namespace skml
