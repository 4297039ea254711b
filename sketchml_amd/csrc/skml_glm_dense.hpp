// skml_glm_dense.hpp -- the tile arithmetic of the dense mini-batch gradient (skml_glm_dense.hip): which
// element of a 64-row x kDenseC-column tile of the row-major x a lane loads, where the transposed
// slab in LDS keeps it, how many columns a partial tile has, and how the waves are grouped.  No device
// builtins: the kernels and the host program tests/glm_dense_check.cpp instantiate the same functions.
#pragma once
#include <stdint.h>

#include "skml_glm.hpp"

namespace skml {

// ---- the row dot: a wave owns 64 consecutive batch positions, a lane one of them ----
constexpr int kDenseC = 16;  // columns of a tile: a row's 128 contiguous bytes, one load of 16 lanes
constexpr int kDenseS = 68;  // doubles between two columns of the slab: 64 rows + 4 of padding
constexpr int kDenseLoads = kDenseC;                 // loads a lane makes per tile: 64 * C / 64
constexpr int kDenseRowsPerLoad = 64 / kDenseC;      // rows one load instruction of the wave covers
constexpr int kDenseSlab = kDenseC * kDenseS;        // doubles of one slab
constexpr int kDenseWaveLds = 2 * kDenseSlab * 8;    // bytes of LDS per wave: two slabs
constexpr int kDenseMaxWaves = 2;                    // waves per workgroup: 1 or 2

// Load i (0 .. kDenseLoads) of `lane`: the tile's row (0 .. 64) and column (0 .. kDenseC).  The 16 lanes
// of a row read consecutive doubles.
SKML_GLM_HD int dense_load_row(int i, int lane) { return i * kDenseRowsPerLoad + lane / kDenseC; }
SKML_GLM_HD int dense_load_col(int lane) { return lane % kDenseC; }
// The slab keeps the tile transposed: column c of row r at c * kDenseS + r.  The chain's reads (lane =
// row, one column) are 64 consecutive doubles; the stores of one load instruction land on
// 4 * col + (lane / 16) + 4 * i mod 64: 64 different 8-byte words, so neither side has a bank conflict.
SKML_GLM_HD int dense_slab_index(int col, int row) { return col * kDenseS + row; }
// Columns of the tile at c0: an exact trip count, so a partial tile adds nothing.
SKML_GLM_HD int dense_tile_cols(int64_t dim, int64_t c0) {
    const int64_t rem = dim - c0;
    return rem >= kDenseC ? kDenseC : (rem > 0 ? (int)rem : 0);
}
// Waves of 64 batch positions, and how many share a workgroup: one while the waves are few, so that
// they spread over the compute units; two from kDenseGroupAt waves on.
constexpr int64_t kDenseGroupAt = 2048;
SKML_GLM_HD int64_t dense_row_waves(int64_t batch) { return (batch + 63) / 64; }
SKML_GLM_HD int dense_waves_per_group(int64_t waves) { return waves >= kDenseGroupAt ? kDenseMaxWaves : 1; }

// ---- the column sum: a wave owns 64 * kDenseV consecutive columns, a lane kDenseV of them ----
constexpr int kDenseU = 32;  // rows of loads in flight ahead of the dependent add
constexpr int kDenseV = 1;   // columns per lane
constexpr int kDenseWaveCols = 64 * kDenseV;
// Column v of `lane` in the wave that starts at column `base`: the lanes of one load are consecutive.
SKML_GLM_HD int64_t dense_col_of(int64_t base, int v, int lane) { return base + (int64_t)v * 64 + lane; }
SKML_GLM_HD int64_t dense_col_waves(int64_t dim) { return (dim + kDenseWaveCols - 1) / kDenseWaveCols; }
// Threads of a workgroup of the column sum: one wave while they are few, four from kDenseColGroupAt on.
constexpr int64_t kDenseColGroupAt = 1024;
SKML_GLM_HD int dense_col_threads(int64_t waves) { return waves >= kDenseColGroupAt ? 256 : 64; }

}  // namespace skml
