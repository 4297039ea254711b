"""GPU parity of the sketch leaf's bookkeeping: the RNG jump on the scalar unit, the per-wave
min / max / flags without a cross-lane reduction of the flags, the draw-bit selectors and the last
merge pass, each against the CPU restatement byte for byte (header, splits, every bin, every decoded
float), the way tests/test_gpu_dense.py compares.

Layout the plantings rely on: a leaf tile is 64 chunks of 256 floats (16,384 floats); the split leaf
gives round r of a tile (chunks 16 r .. 16 r + 15) to wave r of the workgroup, 4 lanes per chunk.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

CHUNK = 256
ROUND = 16 * CHUNK
TILE = 64 * CHUNK
N20 = 2**20  # 64 tiles


def _check_small(gpu, x, seed):
    """Whole-payload parity through the one-call oracle (sizes up to ~10 M floats)."""
    gq = gpu.QuantileQuantizer(256, seed=seed)
    gq.quantize(torch.from_numpy(x).cuda())
    oq = O.quantize(x.astype(np.float64), 256, seed)
    assert gq.getBinNum() == oq.bin_num
    assert gq.getZeroIdx() == oq.zero_idx
    assert gq.getMin() == oq.min and gq.getMax() == oq.max
    gs = gq.getSplits()
    assert gs.shape == oq.splits.shape and np.array_equal(gs.view(np.uint64), oq.splits.view(np.uint64))
    assert np.array_equal(gq.getBins().cpu().numpy(), oq.bins)
    want = oq.values()[oq.bins].astype(np.float32)
    assert np.array_equal(gq.decode().cpu().numpy().view(np.uint32), want.view(np.uint32))
    return oq


def _check_large(gpu, x, seed, slice_n=2**22):
    """The same parity for tens of millions of floats: the oracle's sketch runs once (one Random
    stream, sequential by nature), its quantizeToBins slice by slice on a thread pool."""
    gq = gpu.QuantileQuantizer(256, seed=seed)
    gq.quantize(torch.from_numpy(x).cuda())
    oq = O.quantize_header_f32(x, 256, seed)
    assert gq.getBinNum() == oq.bin_num
    assert gq.getZeroIdx() == oq.zero_idx
    assert gq.getMin() == oq.min and gq.getMax() == oq.max
    gs = gq.getSplits()
    assert gs.shape == oq.splits.shape and np.array_equal(gs.view(np.uint64), oq.splits.view(np.uint64))
    gb = gq.getBins().cpu().numpy()
    dec = gq.decode().cpu().numpy().view(np.uint32)
    vals32 = oq.values().astype(np.float32)

    def check(s0):
        ob = O.index_of_many_f32(oq, x[s0:s0 + slice_n])
        return bool(np.array_equal(gb[s0:s0 + len(ob)], ob)
                    and np.array_equal(dec[s0:s0 + len(ob)], vals32[ob].view(np.uint32)))

    starts = list(range(0, len(x), slice_n))
    with ThreadPoolExecutor(16) as ex:
        bad = [s0 for s0, ok in zip(starts, ex.map(check, starts)) if not ok]
    assert not bad, f"slices differing from the oracle start at {bad[:8]}"


# ---------------------------------------------------------------------------------------------
# 1. jump-table bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2**23 + 2**20, 2**23 + 3 * 2**16 + 70001], ids=["full_tiles", "ragged"])
def test_jump_table_levels_0_1_2(gpu, n):
    """The first draw of a round is #(2 c0 - popcount(c0)) of the stream and the leaf jumps to it
    through a byte-indexed table, one level per byte of the index.  Level 2 is used from draw
    65,536 on, i.e. from chunk ~2^15 (2^23 floats); these sizes run 4,096 and more rounds beyond
    it, so rounds whose index has non-zero bytes at levels 0, 1 and 2 at once (and rounds with a
    zero byte at level 0 or 1, which read the identity entry) all occur.  The second size is
    ragged: full tiles, a partial tile of 17 chunks (levels 4 and 0 of the small trees, run by
    the 32-keys-per-lane leaf, which jumps the same way) and a 113-float tail.  Level 3 needs more
    than 2^31 floats in one bucket; only test_c5_whole_gradient_2p30_matches_oracle comes near
    it, and no test reaches it."""
    c_last = n // CHUNK - 16
    assert 2 * c_last - bin(c_last).count("1") + 1 >= 65536 + 256  # level 2 and below in use
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    _check_small(gpu, x, 40 + n % 7)


# ---------------------------------------------------------------------------------------------
# 2. / 3. plantings
# ---------------------------------------------------------------------------------------------
TILES = {"first": 0, "middle": 31, "last": 63}


def _positions(tile):
    """First and last value of the first and last chunk of each of the tile's four rounds."""
    base = tile * TILE
    return [base + r * ROUND + c * CHUNK + e for r in range(4) for c in (0, 15) for e in (0, CHUNK - 1)]


@pytest.fixture(scope="module")
def base20():
    x = np.random.default_rng(2020).standard_normal(N20).astype(np.float32)
    x[x == 0] = 1.0  # no zero of either sign, so the planted ones are the only ones
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("tile", list(TILES), ids=list(TILES))
@pytest.mark.parametrize("what", ["min", "max"])
def test_extreme_in_every_lane_class(gpu, base20, what, tile):
    """The bucket's single minimum (and, separately, its single maximum) planted in turn at 16
    positions of one tile: whichever wave, chunk and lane holds it, the header's min and max (and
    the rest of the payload) are the oracle's.  A chunk minimum ends in register 0 of the chunk's
    first lane and a maximum in register 63 of its last, and the wave reduces them with DPP row
    operations, so the first and last chunks of a round sit at the two ends of that reduction."""
    v = np.float32(-100.0 if what == "min" else 100.0)
    for p in _positions(TILES[tile]):
        x = base20.copy()
        x[p] = v
        oq = _check_small(gpu, x, 11)
        assert (oq.min if what == "min" else oq.max) == float(v)


@pytest.mark.parametrize("tile", list(TILES), ids=list(TILES))
@pytest.mark.parametrize("what", ["neg_zero", "pos_zero"])
def test_single_zero_flag(gpu, base20, what, tile):
    """A single -0.0 (or +0.0) in the bucket: the wave's flags are built from ballots and are no
    longer reduced across lanes, yet the zero's sign reaches the summary (zero_idx and the splits
    around it) from every planted position."""
    v = np.float32(-0.0 if what == "neg_zero" else 0.0)
    for p in _positions(TILES[tile]):
        x = base20.copy()
        x[p] = v
        _check_small(gpu, x, 12)


@pytest.mark.parametrize("tile", list(TILES), ids=list(TILES))
def test_single_nan_flag(gpu, base20, tile):
    """A single NaN anywhere is reported (HeapQuantileSketch.update rejects NaN)."""
    for p in _positions(TILES[tile]):
        x = base20.copy()
        x[p] = np.nan
        gq = gpu.QuantileQuantizer(256, seed=13)
        with pytest.raises(gpu.QuantileSketchException, match="NaN"):
            gq.quantize(torch.from_numpy(x).cuda())


@pytest.mark.parametrize("rounds", [(0, 1), (1, 0), (0, 3), (2, 3), (3, 1)], ids=lambda r: f"neg{r[0]}_pos{r[1]}")
@pytest.mark.parametrize("tile", list(TILES), ids=list(TILES))
@pytest.mark.parametrize("copies", [1, 192], ids=["single", "many"])
def test_mixed_zero_signs_across_waves(gpu, base20, copies, tile, rounds):
    """A -0.0 and a +0.0 in different rounds of one tile: each wave sees one sign only and stays on
    the fast path, and the merge that first joins the two rounds (level 5 or level 6) must take
    the exact path after the handover of the waves' flags through LDS.  With one zero of each
    sign the flags alone decide; with many copies both signs survive their compactions and meet in
    that merge."""
    rn, rp = rounds
    base = TILES[tile] * TILE
    x = base20.copy()
    x[base + rn * ROUND + 7: base + rn * ROUND + 7 + 2 * copies: 2] = -0.0
    x[base + rp * ROUND + 300: base + rp * ROUND + 300 + 2 * copies: 2] = 0.0
    _check_small(gpu, x, 14)


# ---------------------------------------------------------------------------------------------
# 4. the last merge pass
# ---------------------------------------------------------------------------------------------
def test_last_pass_four_nodes_plus_a_tree(gpu):
    """4 * 2^24 + 2^20 floats: the last merge pass joins 4 level-16 nodes in its two-level form (as
    at 2^28, which test_north_star_2p28_matches_oracle covers) with one more tree (level 12) beside
    them.  The oracle's sequential sketch over 68 M values is most of this test's time."""
    n = 4 * 2**24 + 2**20
    x = np.random.default_rng(424).standard_normal(n).astype(np.float32)
    _check_large(gpu, x, 15)


@pytest.mark.parametrize("kind", ["normal", "signed_zero"])
@pytest.mark.parametrize("n", [2**22, 3 * 2**22 + 2**20 + 999], ids=["2p22", "3x2p22_ragged"])
def test_four_node_group_small(gpu, n, kind):
    """The 4-node group at sizes where the oracle is quick.  2^22 floats are 256 leaf tiles: the
    first pass makes 4 level-12 nodes and the last pass is their 4-node merge.  3 * 2^22 + 2^20 + 999
    leaves 12 level-12 nodes, i.e. an 8-node group and a 4-node group that is a tree root, beside
    smaller trees, a partial tile and a tail.  signed_zero (a fifth of the values +0.0, a fifth
    -0.0) sends the 4-node merge through its exact path, which a 2^28 bucket of N(0,1) never takes."""
    rng = np.random.default_rng(n + len(kind))
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "signed_zero":
        r = rng.random(n)
        x[r < 0.2] = 0.0
        x[(r >= 0.2) & (r < 0.4)] = -0.0
    _check_small(gpu, x, 17)


def test_last_pass_generic(gpu):
    """2^24 floats: one level-16 node, so the last pass is no 4-node merge and takes the generic
    path."""
    n = 2**24
    x = np.random.default_rng(224).standard_normal(n).astype(np.float32)
    _check_large(gpu, x, 16)
