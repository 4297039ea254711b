// skml_glm_dense_multi.hpp -- the plan and the index arithmetic of the dense mini-batch gradient for up to 16
// models per pass over x (skml_glm_dense_multi.hip), the GEMM-shaped variant of the blocked order on
// v_mfma_f64_16x16x4_f64: which rows and columns of x a lane of the row dot feeds to which instruction, how a
// long row of a small batch is split over waves, which columns a lane of the column sum owns and how the
// window's rows are cut into blocks.  Everything is a function of the storage width (8, 4 or 2 bytes), the
// number of models K, batch and dim and of the constants below, never of the device: that is what makes the
// order of every sum, and so its bits, the same on every run.  No device builtins: the kernels and the host
// program tests/glm_dense_multi_check.cpp instantiate the same functions.
//
// The partial sums of the column sum are K times the blocked order's, so the floor of the rows of a block grows
// with K (mul_min_rb): they hold at most 1 / kMulWsShare = 1 / 8 of the window's bytes of x for every storage
// and every K (the argument stands at mul_min_rb).
#pragma once
#include <stdint.h>

#include "skml_glm.hpp"

namespace skml {

constexpr int kMulMaxModels = 16;  // the output columns (row dot) or rows (column sum) of one instruction
constexpr int kMulTileRows = 16;   // window rows of one accumulator tile of the row dot
constexpr int kMulK = 4;           // the k extent of the instruction: slots of the row dot, rows of the column sum

// ---- the row dot: a wave owns R tiles of 16 window rows and walks dim, 4 E columns per wave-step ----
constexpr int kMulAcc = 4;                    // accumulators of a wave: R = 4 row tiles, or 1 tile x 2 wave-steps in flight x 2 (a lane's even and odd columns)
constexpr int kMulTeamWaves = 4;              // waves of a workgroup when a row is not split
constexpr int kMulMaxSplit = 8;               // waves one tile's rows are split over at the most
constexpr int64_t kMulRowTargetWaves = 1024;  // one wave per SIMD of 1,024: R = 4 from four times that, S while below it

// ---- the column sum: a lane owns kMulWords 8-byte words of a row, 16 lanes apart; 4 rows per instruction ----
constexpr int kMulWords = 2;                  // a wave reads 256 contiguous bytes of each of its 4 rows per step
constexpr int kMulU = 8;                      // steps of 4 rows whose loads are in flight ahead of their MFMAs
constexpr int64_t kMulRowsPerIter = kMulK * kMulU;
constexpr int64_t kMulFloorRB = 256;          // floor of the rows of a block for any K, a multiple of kMulRowsPerIter
constexpr int64_t kMulColTargetWaves = 2048;  // strips * NB aims at 2 waves per SIMD
constexpr int kMulColWaves = 4;               // waves (strips) of a workgroup of the column sum
constexpr int64_t kMulWsShare = 8;            // the window's bytes of x over the bytes of partial sums, at least
static_assert(kMulFloorRB % kMulRowsPerIter == 0, "a block is whole iterations, but the window's last");

SKML_GLM_HD int mul_elems_per_group(int x_bytes) { return x_bytes == 8 || x_bytes == 4 || x_bytes == 2 ? 16 / x_bytes : 0; }
SKML_GLM_HD int64_t mul_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// k * n * 8 bytes of a model-major array of doubles; false when that leaves an int64 (or an operand is negative).
SKML_GLM_HD bool mul_bytes(int64_t k, int64_t n, int64_t* bytes) {
    if (k < 0 || n < 0) return false;
    if (k != 0 && n > INT64_MAX / 8 / k) return false;
    *bytes = k * n * 8;
    return true;
}

struct MulPlan {
    int tiles_per_wave;  // R: 16-row tiles a wave of the row dot owns, 1 or 4
    int split;           // S: waves that share a tile, 1, 2, 4 or 8 (above 1 only with R = 1)
    int lane_cols;       // E: consecutive columns of one lane per wave-step (one 16-byte load)
    int strip_cols;      // columns of one wave of the column sum
    int64_t rb, nb;      // the column sum: rows per block, blocks
    int64_t ws_bytes;    // nb * K * dim doubles of partial sums, 0 when nb == 1
};

// Wave-steps a wave has in flight per tile.
constexpr int mul_steps_in_flight(int tiles_per_wave) { return tiles_per_wave == 1 ? 2 : 1; }
// Wave-steps of 4 E columns that cover a row.
SKML_GLM_HD int64_t mul_col_steps(int e, int64_t dim) { return mul_ceil_div(dim, (int64_t)kMulK * e); }
SKML_GLM_HD int64_t mul_tiles(int64_t batch) { return mul_ceil_div(batch, kMulTileRows); }
SKML_GLM_HD int mul_tiles_per_wave(int64_t tiles) { return tiles >= kMulAcc * kMulRowTargetWaves ? kMulAcc : 1; }
// Waves a tile's rows are split over: while the launch stays at or below the target and every wave keeps one
// full iteration of its wave-steps in flight.
SKML_GLM_HD int mul_split(int64_t tiles, int64_t steps) {
    int s = 1;
    while (s < kMulMaxSplit && tiles * (2 * s) <= kMulRowTargetWaves && steps >= (int64_t)2 * s * mul_steps_in_flight(1)) s *= 2;
    return s;
}

// Floor of the rows of a block.  With nb >= 2 blocks batch > rb, so nb < 2 * batch / rb and the partial sums
// hold nb * K * dim * 8 < 16 * K * batch * dim / rb bytes; with rb >= 16 * K * kMulWsShare / x_bytes that is at
// most batch * dim * x_bytes / kMulWsShare, the window's bytes of x over kMulWsShare.
SKML_GLM_HD int64_t mul_min_rb(int x_bytes, int models) {
    const int64_t need = mul_ceil_div(mul_ceil_div((int64_t)16 * models * kMulWsShare, x_bytes), kMulRowsPerIter) * kMulRowsPerIter;
    return need < kMulFloorRB ? kMulFloorRB : need;
}
// Columns of one wave of the column sum: kMulWords words of 8 bytes on each of 16 lanes.
SKML_GLM_HD int mul_strip_cols(int x_bytes) { return 16 * kMulWords * (8 / x_bytes); }
SKML_GLM_HD int64_t mul_strips(int x_bytes, int64_t dim) { return mul_ceil_div(dim, mul_strip_cols(x_bytes)); }

// The plan of one call; false for a bad argument.
SKML_GLM_HD bool mul_plan(int x_bytes, int models, int64_t batch, int64_t dim, MulPlan* p) {
    const int e = mul_elems_per_group(x_bytes);
    if (!e || models < 1 || models > kMulMaxModels || batch < 1 || dim < 1 || batch > 0x7FFFFFFFLL || dim > 0x7FFFFFFFLL) return false;
    const int64_t tiles = mul_tiles(batch);
    p->tiles_per_wave = mul_tiles_per_wave(tiles);
    p->split = p->tiles_per_wave == 1 ? mul_split(tiles, mul_col_steps(e, dim)) : 1;
    p->lane_cols = e;
    p->strip_cols = mul_strip_cols(x_bytes);
    const int64_t nb0 = mul_ceil_div(kMulColTargetWaves, mul_strips(x_bytes, dim));
    const int64_t rb = mul_ceil_div(mul_ceil_div(batch, nb0), kMulRowsPerIter) * kMulRowsPerIter, lo = mul_min_rb(x_bytes, models);
    p->rb = rb < lo ? lo : rb;
    p->nb = mul_ceil_div(batch, p->rb);
    p->ws_bytes = p->nb > 1 ? p->nb * models * dim * 8 : 0;
    return true;
}

// ---- the row dot's walk ----
// Team tm (one wave, or the S waves of a workgroup) owns the tiles tm * R .. tm * R + R - 1; lane `lane` stands
// for batch position tile * 16 + lane % 16 on the x operand and for model lane % 16 on the w operand, both at
// slot q = lane / 16.  In the iteration that starts at wave-step `base` (0, stride, 2 * stride ... below the
// row's wave-steps) wave s takes at slot a (0 .. mul_steps_in_flight(R)) the wave-step below; of that wave-step the
// lane takes the E columns from mul_lane_col on and feeds them to E instructions in turn.
SKML_GLM_HD int64_t mul_teams(const MulPlan& p, int64_t batch) { return mul_ceil_div(mul_tiles(batch), p.tiles_per_wave); }
SKML_GLM_HD int mul_teams_per_group(const MulPlan& p) { return p.split > 1 ? 1 : kMulTeamWaves; }
SKML_GLM_HD int64_t mul_step_stride(const MulPlan& p) { return (int64_t)mul_steps_in_flight(p.tiles_per_wave) * p.split; }
SKML_GLM_HD int64_t mul_step_of(int64_t base, int a, int split, int s) { return base + (int64_t)a * split + s; }
SKML_GLM_HD int64_t mul_lane_col(int64_t step, int q, int e) { return (step * kMulK + q) * e; }
// The batch position of row r (0 .. 4) of the lane's four results of a tile: the instruction's D layout.
// The model of row r of the lane's four results of a tile of the column sum: the same layout.
SKML_GLM_HD int mul_out_model(int lane, int r) { return 4 * r + lane / 16; }
SKML_GLM_HD int64_t mul_out_row(int64_t tile, int lane, int r) { return tile * kMulTileRows + 4 * r + lane / 16; }

// ---- the column sum's walk ----
// First column of word t (0 .. kMulWords) of lane n = lane % 16 of strip `strip`; the word holds V = 8 / XB
// adjacent columns, one accumulator tile each.  A wave's load of word t reads 128 contiguous bytes of each of
// its 4 rows, the kMulWords loads 256.
template <int XB>
SKML_GLM_HD int64_t mul_col_of(int64_t strip, int t, int n) { return ((strip * kMulWords + t) * 16 + n) * (8 / XB); }
// Batch positions [*j0, *j1) of block b; the lane of slot k = lane / 16 takes position j + 4 * u + k at step u of
// the iteration that starts at j (j0, j0 + kMulRowsPerIter ... below j1).
SKML_GLM_HD void mul_block_rows(const MulPlan& p, int64_t batch, int64_t b, int64_t* j0, int64_t* j1) {
    *j0 = b * p.rb;
    *j1 = *j0 + p.rb < batch ? *j0 + p.rb : batch;
}
SKML_GLM_HD int64_t mul_row_pos(int64_t j, int u, int k) { return j + (int64_t)kMulK * u + k; }

}  // namespace skml
