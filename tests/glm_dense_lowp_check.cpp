// skml_glm_dense_lowp.hpp on the host under ASan / UBSan (tests/test_glm_dense_lowp_cpu.py), for both element
// widths: the 64 stores of every store instruction (one element index of one load) touch 64 different
// banks; a tile's loads fill every element and slab slot once and the chain's reads of a column are the 64
// rows in lane order; partial tiles count dim exactly and load only groups inside the pitch; the lanes of
// the column sum's waves own [0, dim) once.
#include <cstdio>
#include <vector>

#include "../sketchml_amd/csrc/skml_glm_dense_lowp.hpp"

using namespace skml;

static int fail(const char* what, long a, long b) {
    std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
    return 1;
}

template <int E>
static int check() {
    using T = LowpTile<E>;
    static_assert(kLowpLoads * kLowpRowsPerLoad == 64 && kLowpGroups * E == T::kC && T::kC % kLowpChunk == 0, "tile");
    static_assert(kLowpMaxWaves * T::kWaveLds <= 65536 && T::kS >= 64, "LDS budget and stride");
    std::vector<int> slot(T::kSlab, 0), elem(64 * T::kC, 0);
    for (int i = 0; i < kLowpLoads; i++)
        for (int e = 0; e < E; e++) {
            unsigned long long banks = 0;
            for (int lane = 0; lane < 64; lane++) {
                const int row = lowp_load_row(i, lane), col = lowp_load_col<E>(lane, e), s = lowp_slab_index<E>(col, row);
                if (row < 0 || row >= 64 || col < 0 || col >= T::kC || s < 0 || s >= T::kSlab) return fail("outside the tile", i, lane);
                if (lane % kLowpGroups && (row != lowp_load_row(i, lane - 1) || col != lowp_load_col<E>(lane - 1, e) + E))
                    return fail("a row's lanes are not consecutive groups", i, lane);
                if (slot[(size_t)s]++ || elem[(size_t)(row * T::kC + col)]++) return fail("filled twice", i, lane);
                banks |= 1ull << (s % 64);
            }
            if (~banks) return fail("store bank conflict", i, e);
        }
    for (int v : elem)
        if (v != 1) return fail("element not loaded", v, 0);
    for (int c = 0; c < T::kC; c++)
        for (int r = 0; r < 64; r++)
            if (lowp_slab_index<E>(c, r) != lowp_slab_index<E>(c, 0) + r || !slot[(size_t)lowp_slab_index<E>(c, r)])
                return fail("reads not consecutive or of an empty slot", c, r);
    for (int64_t dim : {(int64_t)1, (int64_t)T::kC - 1, (int64_t)T::kC, (int64_t)T::kC + 1, (int64_t)2 * T::kC + 3}) {
        const int64_t pitch = (dim + E - 1) / E * E;
        int64_t n = 0;
        for (int64_t c0 = 0; c0 < dim; c0 += T::kC) {
            const int cn = lowp_tile_cols<E>(dim, c0);
            n += cn;
            for (int lane = 0; lane < 64; lane++) {  // a group is loaded whole or not at all, and always where a column is added
                const int64_t first = c0 + lowp_load_col<E>(lane, 0);
                const bool in = lowp_group_in_pitch<E>(pitch, c0, lane);
                if (in != (first + E <= pitch) || (first < c0 + cn && !in)) return fail("group against the pitch", (long)dim, lane);
            }
        }
        if (n != dim || lowp_tile_cols<E>(dim, dim) != 0) return fail("tile columns", (long)dim, (long)n);
    }
    constexpr int V = LowpCols<E>::kV, WC = LowpCols<E>::kWaveCols;
    static_assert(V * (16 / E) == 4 && WC * (16 / E) >= 256, "a lane loads a dword, a wave 256 contiguous bytes");
    for (int64_t dim : {(int64_t)1, (int64_t)WC - 1, (int64_t)WC, (int64_t)WC + 1, (int64_t)2 * WC + 1}) {
        std::vector<int> owned((size_t)dim, 0);
        for (int64_t wave = 0; wave < lowp_col_waves<E>(dim); wave++)
            for (int lane = 0; lane < 64; lane++)
                for (int v = 0; v < V; v++) {
                    const int64_t k = lowp_col_of<E>(wave * WC, v, lane);
                    if (v && k != lowp_col_of<E>(wave * WC, v - 1, lane) + 1) return fail("a lane's columns are not adjacent", lane, v);
                    if (lowp_col_of<E>(wave * WC, 0, lane) % V) return fail("a lane's dword is misaligned", lane, v);
                    if (k < dim) owned[(size_t)k]++;
                }
        for (int o : owned)
            if (o != 1) return fail("column not owned once", (long)dim, o);
        if ((lowp_col_waves<E>(dim) - 1) * WC >= dim) return fail("a wave without a column", (long)dim, 0);
    }
    return 0;
}

int main() {
    if (lowp_elems_per_group(SKML_X_F32) != 4 || lowp_elems_per_group(SKML_X_BF16) != 8 || lowp_elems_per_group(SKML_X_F16) != 8 ||
        lowp_elems_per_group(3) != 0 || lowp_elems_per_group(-1) != 0)
        return fail("elements per group", 0, 0);
    if (lowp_waves_per_group(kLowpGroupAt - 1) != 1 || lowp_waves_per_group(kLowpGroupAt) != kLowpMaxWaves ||
        lowp_col_threads(kLowpColGroupAt - 1) != 64 || lowp_col_threads(kLowpColGroupAt) != 256)
        return fail("workgroup cut-offs", 0, 0);
    if (check<4>() || check<8>()) return 1;
    std::printf("ok\n");
    return 0;
}
