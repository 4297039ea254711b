"""GPU parity of the leaf's in-register sort with its merge phases in 3-input form
(sketchml_amd/csrc/skml_fused_merge.hpp; tests/test_leaf_fused_merge_model.py is the exact CPU check
of the op list): whole payloads against the CPU restatement, byte for byte (header, splits, every
bin, every decoded float), on inputs built per lane.

Layout: a leaf tile is 64 chunks of 256 floats; 4 lanes hold a chunk, and register r = 4 j + e of
lane l (= lane & 3) is the chunk's float 16 j + 4 l + e.  The 64-key sort first sorts blocks of 4
registers, then merges 4+4, 8+8, 16+16 and 32+32 registers."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

CHUNK = 256
TILE = 64 * CHUNK
SIZES = {"one_tile": 1, "64_tiles": 64}


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


def _lanes(tiles):
    return tiles * 64 * 4


def _runs(rng, lanes):
    """Lane i holds, by i % 4: an ascending run, a descending run, an organ pipe (up, then down),
    64 copies of one value.  The values differ from lane to lane."""
    v = np.sort(rng.standard_normal((lanes, 64)).astype(np.float32), axis=1)
    kind = np.arange(lanes) % 4
    v[kind == 1] = v[kind == 1][:, ::-1]
    pipe = np.concatenate([v[:, 0::2], v[:, ::-1][:, 0::2]], axis=1)
    v[kind == 2] = pipe[kind == 2]
    v[kind == 3] = v[kind == 3][:, :1]
    return v


def _split32(rng, lanes):
    """Two distinct values per lane, the low one in za of registers 0..31 and zb of registers
    32..63, at scattered positions: the 32+32 merge then sees the zero-one input (za, zb).  All
    33 * 33 split points occur from 1,089 lanes on (64 tiles have 16,384); one tile takes every
    fourth or fifth of them.  A med3 with a wrong operand gives a wrong order for some (za, zb)."""
    lo = rng.standard_normal(lanes).astype(np.float32)
    hi = lo + np.float32(0.25) + np.abs(rng.standard_normal(lanes)).astype(np.float32)
    pts = [(za, zb) for za in range(33) for zb in range(33)]
    v = np.empty((lanes, 64), dtype=np.float32)
    for i in range(lanes):
        za, zb = pts[(i * len(pts)) // lanes if lanes < len(pts) else i % len(pts)]
        half_a = np.where(rng.permutation(32) < za, lo[i], hi[i])
        half_b = np.where(rng.permutation(32) < zb, lo[i], hi[i])
        v[i] = np.concatenate([half_a, half_b])
    return v


def _input(kind, tiles):
    rng = np.random.default_rng(1000 * tiles + len(kind))
    lanes = _lanes(tiles)
    n = tiles * TILE
    if kind == "runs":
        return _from_lanes(_runs(rng, lanes))
    if kind == "split32":
        return _from_lanes(_split32(rng, lanes))
    if kind == "five_values":
        return rng.choice(np.array([-2.5, -1.0, 0.5, 0.75, 3.0], dtype=np.float32), n)
    x = rng.standard_normal(n).astype(np.float32)
    r = rng.random(n)
    if kind == "inf_denormal":
        x[r < 0.03] = np.inf
        x[(r >= 0.03) & (r < 0.06)] = -np.inf
        x[(r >= 0.06) & (r < 0.12)] = np.float32(1e-40)
        x[(r >= 0.12) & (r < 0.18)] = np.float32(-3e-41)
        x[(r >= 0.18) & (r < 0.22)] = np.float32(1.4e-45)
    elif kind == "both_zero_signs":  # the exact loop: it sorts through the same function
        x[r < 0.1] = 0.0
        x[(r >= 0.1) & (r < 0.2)] = -0.0
    elif kind == "pos_zero_only":
        x[r < 0.1] = 0.0
    elif kind == "neg_zero_only":
        x[r < 0.1] = -0.0
    else:
        raise ValueError(kind)
    return x


KINDS = ["runs", "split32", "five_values", "inf_denormal", "both_zero_signs", "pos_zero_only", "neg_zero_only"]


@pytest.mark.parametrize("size", list(SIZES), ids=list(SIZES))
@pytest.mark.parametrize("kind", KINDS)
def test_per_lane_inputs(gpu, kind, size):
    x = _input(kind, SIZES[size])
    assert x.size == SIZES[size] * TILE
    _check(gpu, x, 21 + len(kind))


def test_split32_covers_every_split_point():
    """The planting itself (no GPU): after sorting each half, lane i of the 64-tile input is the
    zero-one input (za, zb) of the 32+32 merge, and every pair occurs."""
    v = _split32(np.random.default_rng(5), 2 * 33 * 33)
    lo = v.min(axis=1, keepdims=True)
    za = (v[:, :32] == lo).sum(axis=1)
    zb = (v[:, 32:] == lo).sum(axis=1)
    two = (v.max(axis=1) > v.min(axis=1))  # (0, 0) and (32, 32) are the lanes of one value
    assert len(set(zip(za[two].tolist(), zb[two].tolist()))) == 33 * 33 - 2
    assert (~two).sum() == 2 * 2
    x = _from_lanes(v[:4])
    assert np.array_equal(x.reshape(16, 4, 4)[:, 1, :].reshape(-1), v[1])  # lane 1: floats 16 j + 4 + e


def test_normal_2p22_fast_loop(gpu):
    """2^22 N(0,1) floats: 256 tiles, the fast loop for many rounds, and the 4-node last merge."""
    x = np.random.default_rng(222).standard_normal(2**22).astype(np.float32)
    _check(gpu, x, 23)


def test_bf16_input(gpu):
    """bf16 storage is widened in the leaf's load and sorted by the same function; N(0,1) rounded
    to bf16 has heavy ties."""
    x = np.random.default_rng(16).standard_normal(16 * TILE + 5 * CHUNK + 77).astype(np.float32)
    x16 = torch.from_numpy(x).to(torch.bfloat16)
    _check(gpu, x16.float().numpy(), 24, xt=x16)


@pytest.mark.parametrize("kind", ["normal", "both_zero_signs"])
def test_ragged_partial_tile(gpu, kind):
    """8 full tiles, a partial tile of 17 chunks and a 113-float tail: the partial tile is sorted
    32 keys per lane (sort_regs_oddeven<32>, the R = 32 list), in its fast loop or its exact one."""
    n = 8 * TILE + 17 * CHUNK + 113
    rng = np.random.default_rng(n + len(kind))
    x = rng.standard_normal(n).astype(np.float32)
    x[rng.random(n) < 0.05] = 1.5
    if kind == "both_zero_signs":
        r = rng.random(n)
        x[r < 0.1] = 0.0
        x[(r >= 0.1) & (r < 0.2)] = -0.0
    _check(gpu, x, 25)
