"""The quantize pass's self-built bucket table (skml_dense.hip k_quantize with no table passed: each
workgroup builds it in LDS from the payload's splits, with byte entries for a request of <= 256
bins and 16-bit entries otherwise), compared byte for byte with

* the passed-table form: the same input re-encoded by skml_dense_encode_with_splits_f32 with the
  splits read back from the first payload (k_set_splits builds a global 16-bit table, the pass
  copies it) must give identical code bytes; needs no reference;
* the CPU oracle, with the checks the other dense tests use.

Shapes: one value, one short of a tile, one tile, tiles + a tail, several workgroups; 2^23 + 5 for
a grid past 1,024 workgroups with more than one tile per wave.  Inputs: 2 / 4 bins (1- and 2-bit
codes), 256 / 257 requested bins (the byte / 16-bit entry boundary), few distinct values inside one bucket (cmax > 15: the
Eytzinger table written over the table just built), both zero signs with a split at zero, integers
(every value equals a split), a NaN (the encode refuses it, like the oracle), bf16 / fp16 input.

255 splits, the top of a byte entry: a sketch level holds 128 samples, so how many of the 255 ranks
land on distinct samples depends on the levels n fills, not on the values.  n = 70,001 (levels 0, 4
and 8) gives 148 bins for any input and 2^23 + 5 (one level) 133; n = 2^17 - 1 fills levels 0 to 8
and the base buffer, and its more than 65,536 distinct values give all 256 bins (N255; so does
n = 1,023, below one full level).  Both are asserted.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [1, 1023, 1024, 4096 + 7, 70001]
BIG = 2**23 + 5
N255 = 2**17 - 1
# (kind, requested bins)
CASES = [("normal", 2), ("normal", 4), ("normal", 256), ("normal", 257), ("ints", 4), ("ints", 256),
         ("zeros", 4), ("zeros", 256), ("cluster", 256), ("cluster", 257)]
SEED = 5


def _values(n, kind):
    rng = np.random.default_rng(977 * n + len(kind))
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "ints":  # every split is one of the values: the `<=` compare at a split
        return rng.integers(-5, 6, n).astype(np.float32)
    if kind == "zeros":  # splits at zero, values of both zero signs
        x = rng.standard_normal(n).astype(np.float32)
        r = rng.random(n)
        x[r < 0.3] = 0.0
        x[(r >= 0.3) & (r < 0.6)] = -0.0
        return x
    if kind == "cluster":  # 40 distinct values inside one table bucket ([1, 1 + 1/32)): cmax > 15
        return (np.float32(1.0) + rng.integers(0, 40, n).astype(np.float32) * np.float32(2.0**-20)).astype(np.float32)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _case(n, kind, bins):
    """Input and oracle result of one encode, computed once and shared (never modified)."""
    x = _values(n, kind)
    x.setflags(write=False)
    return x, O.quantize(x.astype(np.float64), bins, SEED)


def _codes(q):
    """The code bytes of q's payload."""
    h = q._load_header()
    nbytes = (q.n * h.code_bits + 7) // 8
    return q.payload[h.codes_offset:h.codes_offset + nbytes].cpu().numpy()


def _encode_passed_table(gpu, x32, q):
    """x32 re-encoded against q's split table by the set-splits entry; its code bytes."""
    from sketchml_amd import _lib
    h = q._load_header()
    sp = np.ascontiguousarray(q.getSplits(), dtype=np.float64)
    assert len(sp) == h.bin_num - 1 and len(sp) >= 1
    n = x32.numel()
    nb = _lib.lib.skml_dense_payload_bytes(n, len(sp) + 1)
    pl = gpu.alloc_aligned(nb, "cuda")
    ctx = gpu.get_context()
    st = _lib.lib.skml_dense_encode_with_splits_f32(ctx.handle, C.c_void_p(x32.data_ptr()), n, sp.ctypes.data_as(_lib.dblp),
                                                    len(sp), h.min, h.max, C.c_void_p(pl.data_ptr()), nb)
    assert st == 0, _lib.last_error()
    h2 = _lib.DenseHeader()
    assert _lib.lib.skml_dense_info(ctx.handle, C.c_void_p(pl.data_ptr()), C.byref(h2), None, 0) == 0
    assert h2.bin_num == h.bin_num and h2.code_bits == h.code_bits
    return pl[h2.codes_offset:h2.codes_offset + (n * h2.code_bits + 7) // 8].cpu().numpy()


def _check_oracle(gq, oq):
    assert gq.getBinNum() == oq.bin_num
    assert gq.getZeroIdx() == oq.zero_idx
    assert gq.getMin() == oq.min and gq.getMax() == oq.max
    gs = gq.getSplits()
    assert gs.shape == oq.splits.shape
    assert np.array_equal(gs.view(np.uint64), oq.splits.view(np.uint64)) or np.array_equal(gs, oq.splits)
    assert np.array_equal(gq.getBins().cpu().numpy(), oq.bins)
    dec = gq.decode().cpu().numpy()
    want = oq.values()[oq.bins].astype(np.float32)
    assert np.array_equal(dec.view(np.uint32), want.view(np.uint32))


def _encode(gpu, x, bins):
    q = gpu.QuantileQuantizer(bins, seed=SEED)
    q.quantize(x)
    return q


def _assert_reaches_its_branch(q, n, kind, bins):
    """The input is what it is for.  normal / 256 bins at the sizes named above: the payload really
    carries 255 splits, so the byte table's last bases are 255.  cluster: more than kLutMaxNeed = 15 splits share one
    bucket (the top 14 bits of a float's key), so the build ends in the Eytzinger mode."""
    if kind == "normal" and bins == 256 and n in (1023, N255):
        assert q.getBinNum() == 256
    if kind == "cluster" and n >= 4096:
        keys = q.getSplits().astype(np.float32).view(np.uint32) >> 18  # positive floats: key order = bit order
        assert np.bincount(keys - keys.min()).max() > 15


@pytest.mark.parametrize("kind,bins", CASES)
@pytest.mark.parametrize("n", SHAPES)
def test_self_built_equals_passed_table(gpu, n, kind, bins):
    x = torch.from_numpy(_values(n, kind)).cuda()
    q = _encode(gpu, x, bins)
    _assert_reaches_its_branch(q, n, kind, bins)
    assert np.array_equal(_codes(q), _encode_passed_table(gpu, x, q))


@pytest.mark.parametrize("kind,bins", CASES)
@pytest.mark.parametrize("n", SHAPES)
def test_self_built_matches_oracle(gpu, n, kind, bins):
    x, oq = _case(n, kind, bins)
    q = _encode(gpu, torch.from_numpy(x).cuda(), bins)
    _assert_reaches_its_branch(q, n, kind, bins)
    _check_oracle(q, oq)


@pytest.mark.parametrize("bins", [256, 257])
def test_more_than_1024_workgroups(gpu, bins):
    """2^23 + 5 values: 8,193 tiles, so the grid passes 1,024 workgroups where the device holds
    more, and every wave takes more than one tile."""
    x, oq = _case(BIG, "normal", bins)
    xt = torch.from_numpy(x).cuda()
    q = _encode(gpu, xt, bins)
    _assert_reaches_its_branch(q, BIG, "normal", bins)
    _check_oracle(q, oq)
    assert np.array_equal(_codes(q), _encode_passed_table(gpu, xt, q))


def test_byte_entries_reach_255(gpu):
    """256 requested bins and more than 65,536 distinct values whose payload carries all 255 splits."""
    x, oq = _case(N255, "normal", 256)
    assert len(np.unique(x)) >= 65536 and oq.bin_num == 256
    xt = torch.from_numpy(x).cuda()
    q = _encode(gpu, xt, 256)
    _assert_reaches_its_branch(q, N255, "normal", 256)
    _check_oracle(q, oq)
    assert np.array_equal(_codes(q), _encode_passed_table(gpu, xt, q))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind,bins", [("normal", 256), ("zeros", 4)])
def test_sixteen_bit_input(gpu, dt, kind, bins):
    n = 4096 + 7
    x16 = torch.from_numpy(_values(n, kind)).to(dt)
    wide = x16.float()
    q = _encode(gpu, x16.cuda(), bins)
    _check_oracle(q, O.quantize(wide.numpy().astype(np.float64), bins, SEED))
    assert np.array_equal(_codes(q), _encode_passed_table(gpu, wide.cuda(), q))


@pytest.mark.parametrize("n,pos", [(4096 + 7, 0), (4096 + 7, 4096 + 6), (70001, 33333)])
def test_nan_among_the_values(gpu, n, pos):
    """A NaN makes the sketch refuse the input (the oracle does too): the quantize pass sees the
    payload's status and builds nothing; the same buffer without the NaN then encodes as usual."""
    x = _values(n, "normal").copy()
    good = x[pos]
    x[pos] = np.nan
    with pytest.raises(O.OracleError):
        O.quantize(x.astype(np.float64), 256, SEED)
    with pytest.raises(gpu.QuantileSketchException):
        _encode(gpu, torch.from_numpy(x).cuda(), 256)
    x[pos] = good
    _check_oracle(_encode(gpu, torch.from_numpy(x).cuda(), 256), _case(n, "normal", 256)[1])
