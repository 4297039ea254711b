// skml_glm_dense.hpp on the host under ASan / UBSan (tests/test_glm_dense_cpu.py): a tile's loads fill every
// element and slab slot once; the 64 stores of a load instruction and the 64 reads of a column touch 64
// different 8-byte words modulo 64 (no bank conflict at any width); partial tiles count dim exactly.
#include <cstdio>
#include <vector>

#include "../sketchml_amd/csrc/skml_glm_dense.hpp"

using namespace skml;

static int fail(const char* what, long a, long b) {
    std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
    return 1;
}

int main() {
    static_assert(kDenseLoads * 64 == 64 * kDenseC && kDenseMaxWaves * kDenseWaveLds <= 65536, "tile and LDS budget");
    std::vector<int> slot(kDenseSlab, 0), elem(64 * kDenseC, 0);
    for (int i = 0; i < kDenseLoads; i++) {
        unsigned long long words = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int row = dense_load_row(i, lane), col = dense_load_col(lane), s = dense_slab_index(col, row);
            if (row < 0 || row >= 64 || col < 0 || col >= kDenseC || s < 0 || s >= kDenseSlab) return fail("outside the tile", i, lane);
            if (lane % kDenseC && (row != dense_load_row(i, lane - 1) || col != dense_load_col(lane - 1) + 1))
                return fail("a row's lanes are not consecutive", i, lane);
            if (slot[(size_t)s]++ || elem[(size_t)(row * kDenseC + col)]++) return fail("filled twice", i, lane);
            words |= 1ull << (s % 64);
        }
        if (~words) return fail("store bank conflict", i, 0);
    }
    for (int e : elem)
        if (e != 1) return fail("element not loaded", e, 0);
    for (int c = 0; c < kDenseC; c++)
        for (int r = 1; r < 64; r++)
            if (dense_slab_index(c, r) != dense_slab_index(c, 0) + r) return fail("reads not consecutive", c, r);
    for (int64_t dim : {(int64_t)1, (int64_t)kDenseC - 1, (int64_t)kDenseC, (int64_t)2 * kDenseC + 3}) {
        int64_t n = 0;
        for (int64_t c0 = 0; c0 < dim; c0 += kDenseC) n += dense_tile_cols(dim, c0);
        if (n != dim || dense_tile_cols(dim, dim) != 0) return fail("tile columns", (long)dim, (long)n);
    }
    std::printf("ok\n");
    return 0;
}
