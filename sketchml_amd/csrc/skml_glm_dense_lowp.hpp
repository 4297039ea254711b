// skml_glm_dense_lowp.hpp -- the tile and column arithmetic of the dense mini-batch gradient over an x stored
// as fp32, bf16 or fp16 (skml_glm_dense_lowp.hip).  Everything is a function of E, the elements of one
// 16-byte load: 4 for fp32, 8 for the 16-bit types.  A row of x starts on a 16-byte boundary (the pitch
// rule of skml_glm_dense_lowp_data), so a lane loads 16 bytes at a time and a tile is 64 rows x 128
// contiguous bytes whatever the type.  No device builtins: the kernels and the host program
// tests/glm_dense_lowp_check.cpp instantiate the same functions.
#pragma once
#include <stdint.h>

#include "../../include/skml.h"
#include "skml_glm.hpp"

namespace skml {

// Elements of one 16-byte group of an x of kind x_kind (SKML_X_*); 0 for an unknown kind.
SKML_GLM_HD int lowp_elems_per_group(int x_kind) {
    return x_kind == SKML_X_F32 ? 4 : (x_kind == SKML_X_BF16 || x_kind == SKML_X_F16 ? 8 : 0);
}

// ---- the row dot: a wave owns 64 consecutive batch positions, a lane one of them ----
constexpr int kLowpGroups = 8;                      // 16-byte groups of a tile's row: 128 bytes
constexpr int kLowpRowsPerLoad = 64 / kLowpGroups;  // rows one load instruction of the wave covers
constexpr int kLowpLoads = 64 / kLowpRowsPerLoad;   // 16-byte loads a lane makes per tile
constexpr int kLowpMaxWaves = 2;                    // waves per workgroup: 1 or 2
constexpr int kLowpChunk = 16;                      // columns of a full tile the chain runs unrolled at a time

template <int E>
struct LowpTile {
    static_assert(E == 4 || E == 8, "16-byte groups of 4-byte or 2-byte elements");
    static constexpr int kC = kLowpGroups * E;  // columns of a tile: 32 or 64
    // dwords between two columns of the slab.  Store instruction e of load i puts lane's element at
    // (E * (lane % 8) + e) * kS + 8 * i + lane / 8: kS * E = 8 mod 64 makes that 8 * (lane % 8) + lane / 8
    // plus a wave-uniform term, a bijection of the 64 lanes onto the 64 banks.
    static constexpr int kS = E == 4 ? 66 : 65;
    static constexpr int kSlab = kC * kS;       // dwords of the slab: 8,448 or 16,640 bytes
    static constexpr int kWaveLds = kSlab * 4;  // bytes of LDS per wave: one slab
};

// Load i (0 .. kLowpLoads) of `lane`: the tile's row (0 .. 64) and 16-byte group (0 .. 8) of that row.
// The 8 lanes of a row read 128 consecutive bytes.
SKML_GLM_HD int lowp_load_row(int i, int lane) { return i * kLowpRowsPerLoad + lane / kLowpGroups; }
SKML_GLM_HD int lowp_load_group(int lane) { return lane % kLowpGroups; }
// The tile's column of element e (0 .. E) of the lane's group.
template <int E>
SKML_GLM_HD int lowp_load_col(int lane, int e) { return E * lowp_load_group(lane) + e; }
// The slab keeps the tile transposed, one dword per element: column c of row r at c * kS + r, so the
// chain's reads (lane = row, one column) are 64 consecutive dwords.
template <int E>
SKML_GLM_HD int lowp_slab_index(int col, int row) { return col * LowpTile<E>::kS + row; }
// Whether the lane's group of the tile at c0 lies inside the pitch: it is loaded whole then, pad elements
// included (they reach the slab and no sum); beyond the pitch the lane loads nothing.
template <int E>
SKML_GLM_HD bool lowp_group_in_pitch(int64_t pitch, int64_t c0, int lane) { return c0 + E * lowp_load_group(lane) < pitch; }
// Columns of the tile at c0 the chain adds: an exact trip count, so neither a pad element nor a column
// past dim reaches a sum.
template <int E>
SKML_GLM_HD int lowp_tile_cols(int64_t dim, int64_t c0) {
    const int64_t rem = dim - c0;
    return rem >= LowpTile<E>::kC ? LowpTile<E>::kC : (rem > 0 ? (int)rem : 0);
}
// Waves of 64 batch positions, and how many share a workgroup: one while they are few, two from
// kLowpGroupAt waves on (the double kernels' cut).
constexpr int64_t kLowpGroupAt = 2048;
SKML_GLM_HD int64_t lowp_row_waves(int64_t batch) { return (batch + 63) / 64; }
SKML_GLM_HD int lowp_waves_per_group(int64_t waves) { return waves >= kLowpGroupAt ? kLowpMaxWaves : 1; }

// ---- the column sum: a lane owns the V adjacent columns of one 4-byte load, a wave 64 * V columns ----
constexpr int kLowpU = 64;  // rows of loads in flight ahead of the dependent adds
template <int E>
struct LowpCols {
    static constexpr int kV = E / 4;  // columns per lane: 1 fp32 or 2 16-bit values in a dword
    static constexpr int kWaveCols = 64 * kV;
};
// Column v of `lane` in the wave that starts at column `base`: a wave's load reads 256 contiguous bytes.
template <int E>
SKML_GLM_HD int64_t lowp_col_of(int64_t base, int v, int lane) { return base + (int64_t)lane * LowpCols<E>::kV + v; }
template <int E>
SKML_GLM_HD int64_t lowp_col_waves(int64_t dim) { return (dim + LowpCols<E>::kWaveCols - 1) / LowpCols<E>::kWaveCols; }
// Threads of a workgroup of the column sum: one wave while they are few, four from kLowpColGroupAt on.
constexpr int64_t kLowpColGroupAt = 1024;
SKML_GLM_HD int lowp_col_threads(int64_t waves) { return waves >= kLowpColGroupAt ? 256 : 64; }

}  // namespace skml
