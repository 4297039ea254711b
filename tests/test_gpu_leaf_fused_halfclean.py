"""GPU parity of the leaf with its in-register half-clean stages in the paired 3-input form
(sketchml_amd/csrc/skml_halfclean.hpp; tests/test_leaf_fused_halfclean_cpu.py is the exact host check
of the template): whole payloads against the CPU restatement, byte for byte (header, splits, every
bin, every decoded float), on inputs built per lane.  The library under test is the loaded one: the
product, or the A/B build (plain stages) when SKML_LIB names it.

Layout: a leaf tile is 64 chunks of 256 floats; 4 lanes hold a chunk, and register r = 4 j + e of
lane l (= lane & 3) is the chunk's float 16 j + 4 l + e.  After the in-lane sort of 64 registers,
lanes 2p and 2p + 1 merge their runs (64 + 64: a flip across the lanes, then six half-clean stages
in registers), then the chunk's two 128-runs merge (128 + 128: a flip, one cross-lane stage, five
stages in registers and the compaction)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

gpu_test = pytest.mark.gpu  # (the planting check below needs no GPU)

CHUNK = 256
TILE = 64 * CHUNK


def _check(gpu, x, seed, xt=None):
    """Whole-payload parity through the one-call oracle; xt: the tensor to encode when it is not x."""
    gq = gpu.QuantileQuantizer(256, seed=seed)
    gq.quantize((torch.from_numpy(x) if xt is None else xt).cuda())
    oq = O.quantize(x.astype(np.float64), 256, seed)
    assert gq.getBinNum() == oq.bin_num
    assert gq.getZeroIdx() == oq.zero_idx
    assert gq.getMin() == oq.min and gq.getMax() == oq.max
    gs = gq.getSplits()
    assert gs.shape == oq.splits.shape and np.array_equal(gs.view(np.uint64), oq.splits.view(np.uint64))
    assert np.array_equal(gq.getBins().cpu().numpy(), oq.bins)
    want = oq.values()[oq.bins].astype(np.float32)
    assert np.array_equal(gq.decode().cpu().numpy().view(np.uint32), want.view(np.uint32))


def _from_lanes(v):
    """v: (lanes, 64) registers of consecutive lanes (4 per chunk) -> the floats in memory order."""
    lanes = v.shape[0]
    assert lanes % 4 == 0 and v.shape[1] == 64
    return np.ascontiguousarray(v.reshape(lanes // 4, 4, 16, 4).transpose(0, 2, 1, 3)).reshape(-1).astype(np.float32)


def _two_values(rng, groups):
    """Two distinct values per group, different from group to group."""
    lo = rng.standard_normal(groups).astype(np.float32)
    hi = (lo + np.float32(0.25) + np.abs(rng.standard_normal(groups)).astype(np.float32)).astype(np.float32)
    return lo, hi


def _planted(rng, lo, hi, za, zb, half):
    """Per group, two runs of `half` values: the low value at za scattered places of the first run and
    zb of the second, the high value elsewhere -> (groups, 2 * half)."""
    g = len(lo)
    ra = np.argsort(rng.random((g, half)), axis=1)
    rb = np.argsort(rng.random((g, half)), axis=1)
    low = np.concatenate([ra < za[:, None], rb < zb[:, None]], axis=1)
    return np.where(low, lo[:, None], hi[:, None]).astype(np.float32)


def _merge128(rng, tiles, lo_hi=None):
    """Lane pair p holds two values, the low one za times in lane 2p and zb times in lane 2p + 1: the
    64 + 64 merge sees the zero-one input (za, zb), pair p the p-th of the 65 * 65 (cyclically; fewer
    pairs than that take them evenly spaced)."""
    pairs = tiles * 64 * 2
    p = np.arange(pairs) % (65 * 65) if pairs >= 65 * 65 else (np.arange(pairs) * (65 * 65)) // pairs
    lo, hi = _two_values(rng, pairs) if lo_hi is None else lo_hi
    v = _planted(rng, lo, hi, p // 65, p % 65, 64)  # (pairs, 128): lane 2p, then lane 2p + 1
    return _from_lanes(v.reshape(pairs * 2, 64))


def _merge256(rng, tiles, first):
    """Chunk c holds two values, the low one za times in lanes 0, 1 and zb times in lanes 2, 3: the
    128 + 128 merge sees the zero-one input (za, zb), chunk c the (first + c)-th of the 129 * 129."""
    chunks = tiles * 64
    p = first + np.arange(chunks)
    assert p[-1] < 129 * 129
    lo, hi = _two_values(rng, chunks)
    v = _planted(rng, lo, hi, p // 129, p % 129, 128)  # (chunks, 256): lanes 0, 1, then lanes 2, 3
    return _from_lanes(v.reshape(chunks * 4, 64))


def _arranged(rng, tiles, rotate):
    """Per chunk 256 distinct values laid over its lanes (lane l takes places 64 l .. 64 l + 63) as an
    organ pipe: the even ranks rising, then the odd ranks falling; rotated by a place count of the
    chunk's own when `rotate`."""
    chunks = tiles * 64
    s = np.sort(rng.standard_normal((chunks, CHUNK)).astype(np.float32), axis=1)
    assert all(len(np.unique(row)) == CHUNK for row in s)
    pipe = np.concatenate([s[:, 0::2], s[:, ::-1][:, 0::2]], axis=1)
    if rotate:
        rot = rng.integers(1, CHUNK, chunks)
        idx = (np.arange(CHUNK)[None, :] + rot[:, None]) % CHUNK
        pipe = np.take_along_axis(pipe, idx, axis=1)
    return _from_lanes(pipe.reshape(chunks * 4, 64))


@gpu_test
def test_128_merge_every_split_point(gpu):
    """Every (za, zb) in {0..64}^2 of the 64 + 64 merge: 4,225 lane pairs of the 8,192 in 64 tiles."""
    x = _merge128(np.random.default_rng(128), 64)
    assert x.size == 2**20
    _check(gpu, x, 31)


@gpu_test
@pytest.mark.parametrize("first", [0, 129 * 129 - 16384], ids=["low", "high"])
def test_256_merge_every_split_point(gpu, first):
    """Every (za, zb) in {0..128}^2 of the 128 + 128 merge: 16,641 chunks, over two cases of 16,384."""
    x = _merge256(np.random.default_rng(256 + first), 256, first)
    assert x.size == 2**22
    _check(gpu, x, 32)


def test_split_points_are_covered():
    """The planting itself (no GPU): the lane pairs of the 64-tile input are the zero-one inputs
    (za, zb) of the 64 + 64 merge, all 65 * 65 of them; the chunks of the two 256-tile inputs are all
    129 * 129 inputs of the 128 + 128 merge."""
    x = _merge128(np.random.default_rng(128), 64)
    v = x.reshape(-1, 16, 4, 4).transpose(0, 2, 1, 3).reshape(-1, 2, 64)  # (pairs, lane of the pair, register)
    lo = v.min(axis=(1, 2), keepdims=True)
    seen = set(zip((v[:, 0] == lo[:, 0]).sum(axis=1).tolist(), (v[:, 1] == lo[:, 0]).sum(axis=1).tolist()))
    # a pair with no low value planted holds one value only and reads as (64, 64) like the full pair
    assert seen == {(a, b) for a in range(65) for b in range(65)} - {(0, 0)}
    assert len(np.unique(v.reshape(len(v), -1), axis=0)) == len(v)  # the values differ between pairs
    seen = set()
    for first in (0, 129 * 129 - 16384):
        c = _merge256(np.random.default_rng(256 + first), 256, first).reshape(-1, 16, 4, 4).transpose(0, 2, 1, 3)
        c = c.reshape(-1, 2, 128)  # (chunks, lanes 0, 1 | lanes 2, 3, 128 values)
        lo = c.min(axis=(1, 2), keepdims=True)
        seen |= set(zip((c[:, 0] == lo[:, 0]).sum(axis=1).tolist(), (c[:, 1] == lo[:, 0]).sum(axis=1).tolist()))
    assert seen == {(a, b) for a in range(129) for b in range(129)} - {(0, 0)}


@pytest.mark.parametrize("rotate", [False, True], ids=["organ_pipe", "rotated_bitonic"])
@gpu_test
def test_distinct_values_one_tile(gpu, rotate):
    x = _arranged(np.random.default_rng(7 + rotate), 1, rotate)
    assert x.size == TILE
    _check(gpu, x, 33)


@gpu_test
def test_ragged_70001(gpu):
    """4 full tiles, a partial tile of 17 chunks and a 113-float tail: the partial tile runs k_leaf2's
    32 keys per lane (half-clean stages over 32, 16, 8 and 4 registers)."""
    n = 70001
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    x[rng.random(n) < 0.05] = 1.5
    _check(gpu, x, 34)


@gpu_test
def test_bf16_input(gpu):
    """bf16 storage is widened in the leaf's load and merged by the same functions: the 64 + 64
    split points over two tiles (every 16th or 17th of them) and a ragged N(0,1) tail."""
    rng = np.random.default_rng(16)
    x = np.concatenate([_merge128(rng, 2), rng.standard_normal(5 * CHUNK + 77).astype(np.float32)])
    x16 = torch.from_numpy(x).to(torch.bfloat16)
    _check(gpu, x16.float().numpy(), 35, xt=x16)


@gpu_test
def test_both_zero_signs_exact_loop(gpu):
    """Both zero signs send a wave to the exact loop, whose chunk sort and level-0 merge run the same
    in-register stages: every third lane pair of the 64 + 64 split points holds (-0.0, +0.0) as its
    two values, then a ragged N(0,1) tail with zeros of both signs."""
    rng = np.random.default_rng(0)
    pairs = 4 * 64 * 2
    lo, hi = _two_values(rng, pairs)
    lo[::3], hi[::3] = -0.0, 0.0
    t = rng.standard_normal(17 * CHUNK + 113).astype(np.float32)
    r = rng.random(t.size)
    t[r < 0.1] = 0.0
    t[(r >= 0.1) & (r < 0.2)] = -0.0
    x = np.concatenate([_merge128(rng, 4, (lo, hi)), t])
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    _check(gpu, x, 36)
