"""ZipMLQuantizer on the device where tests/test_gpu_zipml.py does not reach, bit for bit throughout:

1. the prefix sums r and t as the correctly rounded exact sums (Python-integer sums, rounded once),
   which the compensated tree of k_zip_scan_dd gives and a plain double tree cannot
   (tests/zip_scan_model.py is the tree in numpy, tests/test_zipml_cpu.py shows model == exact on
   these inputs and plain != exact), constant along a run of zeros;
2. bin counts that are odd (thrNum = B / 2 - (splitNum & 1)), around kZipTail = 4,096 (the hand-off
   from the rounds in global memory to k_zip_finish) and between 4,096 and n;
3. gradient-like inputs: one-signed (zero_idx by min > 0 / max < 0), log-normal, a few huge
   outliers, bf16-rounded, mostly zeros;
4. payloads whose final bin count falls into a narrower code width than the requested one (the codes'
   width follows bin_num, their offset req_bins), through every consumer;
5. the radix sort on keys whose digits are all alike, tile after tile;
6. the two size thresholds above 2^22: the integer scan's second level over the rounds' block
   counts (n > 2^23) and its third level over the sort's digit counts (n > 2^27).

The split search is compared with the restatement (tests/zipml_ref.py) run on the device's own sorted
copy and prefix sums, as in tests/test_gpu_zipml.py; every listed case is one the restatement
terminates on, so a refusal fails the test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import zip_scan_model as M
from tests import zipml_ref as Z
from tests.test_gpu_zipml import KINDS, SIZES, _bits, _check_search, _ctx, _dev, _gauss, _hook, _L, _parse, _ptr

pytestmark = pytest.mark.gpu


# ---- 1. prefix sums: correctly rounded ----
@functools.lru_cache(maxsize=None)
def _scan_input(name, n):
    if name == "mostly_zeros":
        return Z.mostly_zeros(n, 1)
    return Z.bf16_rounded(_gauss(n, "f32")).astype(np.float64)


def _check_exact_sums(x):
    s, r, t = _hook(x)
    assert np.array_equal(_bits(s), _bits(Z.java_sort(x.astype(np.float64))))
    er, et = M.exact_prefix_sums(s)
    bad = np.nonzero(_bits(r) != _bits(er))[0]
    assert not len(bad), f"r: {len(bad)} of {len(x)} are not the correctly rounded sum, first at {bad[0]}"
    bad = np.nonzero(_bits(t) != _bits(et))[0]
    assert not len(bad), f"t: {len(bad)} of {len(x)} are not the correctly rounded sum, first at {bad[0]}"
    return s, r, t


@pytest.mark.parametrize("n,kind", [(n, k) for n in SIZES for k in KINDS] + [((1 << 22) + 1, "f32")])
def test_prefix_sums_are_correctly_rounded(n, kind):
    _check_exact_sums(_gauss(n, kind))


@pytest.mark.parametrize("n", [4097, 65539])
@pytest.mark.parametrize("name", ["mostly_zeros", "bf16"])
def test_prefix_sums_are_correctly_rounded_on_runs(name, n):
    s, r, t = _check_exact_sums(_scan_input(name, n))
    if name == "mostly_zeros":
        run = np.nonzero(s == 0)[0]
        assert len(run) > 0.85 * n and run[-1] - run[0] + 1 == len(run)
        assert len(np.unique(_bits(r[run]))) == 1 and len(np.unique(_bits(t[run]))) == 1


# ---- 2 + 3. the split search ----
def _full_search(x, bins):
    """_check_search's header, min, max, splits and zero_idx, then the codes and the rounds."""
    res = _check_search(x, bins)
    assert res is not None, "the restatement terminates on this input"
    h, sp, got, z, pl = res
    assert 2 <= z.bin_num <= min(len(x), bins) and z.rounds == _L().lib.skml_debug_zip_rounds(_ctx().handle)
    assert np.array_equal(got, z.bins(x))
    return h, sp, got, z, pl


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bins", [5, 6, 7, 17, 100, 255, 257, 1000, 4095, 4096, 4097, 5000])
@pytest.mark.parametrize("n", [257, 4097, 8193, 65539])
def test_bin_counts(n, bins, kind):
    _full_search(_gauss(n, kind), bins)


@functools.lru_cache(maxsize=None)
def _input(name, n):
    g = _gauss(n, "f32")
    if name == "positive":
        return np.abs(g) + np.float32(1e-6)
    if name == "negative":
        return -_input("positive", n)
    if name == "lognormal":
        return np.random.default_rng(n).lognormal(0, 2, n).astype(np.float32)
    if name == "outliers":
        x = g.copy()
        x[::n // 7] *= 1e6
        return x
    if name == "bf16":
        return Z.bf16_rounded(g)
    assert name == "mz2"
    return Z.mostly_zeros(n, 2)  # fp64


@pytest.mark.parametrize("bins", [16, 255, 256, 1000, 5000])
@pytest.mark.parametrize("n", [4097, 65539])
@pytest.mark.parametrize("name", ["positive", "negative", "lognormal", "outliers"])
def test_input_kinds(name, n, bins):
    x = _input(name, n)
    assert x.dtype == np.float32
    h, *_ = _full_search(x, bins)
    if name == "positive":
        assert h.min > 0 and h.zero_idx == 0
    if name == "negative":
        assert h.max < 0 and h.zero_idx == h.bin_num - 1


@pytest.mark.parametrize("bins", [16, 17, 256, 257])
@pytest.mark.parametrize("n", [4097, 8193, 65539])
@pytest.mark.parametrize("name", ["bf16", "mz2"])
def test_input_kinds_with_many_ties(name, n, bins):
    x = _input(name, n)
    assert x.dtype == (np.float64 if name == "mz2" else np.float32)
    _full_search(x, bins)


# ---- 4. the final bin count in a narrower code width than the requested one ----
@pytest.mark.parametrize("bins,bin_num,code_bits", [(5, 4, 2), (17, 16, 4), (257, 256, 8)])
def test_consumers_when_bin_num_crosses_a_code_width(bins, bin_num, code_bits):
    import sketchml_amd as sk
    from sketchml_amd.context import alloc_aligned
    L = _L()
    n = 65539
    x, y = _gauss(n, "f32"), _gauss(n + 1, "f32")[:n] * 2
    q = sk.ZipMLQuantizer(bins)
    q.quantize(_dev(x))
    h, sp, got = _parse(q.payload)
    assert (h.req_bins, h.bin_num, h.code_bits) == (bins, bin_num, code_bits)
    z = Z.quantize(x, bins, *_hook(x))
    assert z.bin_num == bin_num and np.array_equal(_bits(sp), _bits(z.splits)) and np.array_equal(got, z.bins(x))
    vals = z.values()
    assert np.array_equal(q.getBins().cpu().numpy(), got)
    assert np.array_equal(q.decode().cpu().numpy(), vals[got].astype(np.float32))
    # writeObject / readObject
    q2 = sk.ZipMLQuantizer.readObject(q.writeObject())
    assert isinstance(q2, sk.ZipMLQuantizer) and np.array_equal(_bits(q2.getSplits()), _bits(sp))
    assert np.array_equal(q2.getBins().cpu().numpy(), got) and (q2.getMin(), q2.getMax()) == (h.min, h.max)
    # decode-sum of two such payloads
    q3 = sk.ZipMLQuantizer(bins)
    q3.quantize(_dev(y))
    h3, sp3, got3 = _parse(q3.payload)
    assert (h3.req_bins, h3.bin_num, h3.code_bits) == (bins, bin_num, code_bits)
    vals3 = Z.ZipResult(Z.OK, h3.bin_num, sp3, h3.min, h3.max, h3.zero_idx).values()
    stride = q.payload.numel()
    assert q3.payload.numel() == stride and stride % 256 == 0
    both = alloc_aligned(2 * stride, "cuda")
    both[:stride].copy_(q.payload)
    both[stride:].copy_(q3.payload)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    assert L.lib.skml_dense_decode_sum_f32(_ctx().handle, _ptr(both), 2, stride, _ptr(out), n, 1.0) == 0, L.last_error()
    assert np.array_equal(out.cpu().numpy(), ((0.0 + vals[got] + vals3[got3]) * 1.0).astype(np.float32))
    # the host's view of the same bytes
    pl = q.payload.cpu().numpy().copy()
    hh = L.DenseHeader()
    hsp = np.zeros(bins, dtype=np.float64)
    assert L.lib.skml_dense_info_host(pl.ctypes.data_as(C.c_void_p), len(pl), C.byref(hh), hsp.ctypes.data_as(L.dblp),
                                      bins) == 0, L.last_error()
    assert bytes(hh) == bytes(h) and np.array_equal(_bits(hsp[: bin_num - 1]), _bits(sp))
    hb = np.zeros(n, dtype=np.int32)
    assert L.lib.skml_dense_bins_host(pl.ctypes.data_as(C.c_void_p), len(pl), hb.ctypes.data_as(C.c_void_p), n) == 0
    assert np.array_equal(hb, got)


# ---- 5. the sort on skewed digits ----
@functools.lru_cache(maxsize=None)
def _skewed(name, n, kind):
    dt = np.float32 if kind == "f32" else np.float64
    if name == "constant":
        return np.full(n, 0.25, dtype=dt)
    if name == "two_values":
        return np.where(np.arange(n) & 1, -0.25, 0.25).astype(dt)
    if name == "ascending":
        return np.sort(_gauss(n, kind))
    if name == "descending":
        return np.sort(_gauss(n, kind))[::-1].copy()
    if name == "f32_values":  # as doubles: the low three digits 0x00 (positive) or 0xFF (negative)
        return _gauss(n, "f32").astype(dt)
    if name == "low_byte":  # 1 + k eps: keys that differ in the lowest digit alone
        return (dt(1.0) + (np.arange(n) % 256).astype(dt) * np.finfo(dt).eps).astype(dt)
    assert name == "high_byte"  # +-2^(16 j): per sign, keys that differ in the highest digit alone
    top = 7 if kind == "f32" else 63
    rng = np.random.default_rng(n)
    j = rng.integers(-top, top + 1, n)
    return (np.ldexp(1.0, 16 * j) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(dt)


SKEWED = [(name, kind) for name in ("constant", "two_values", "ascending", "descending", "low_byte", "high_byte")
          for kind in KINDS] + [("f32_values", "f64")]


@pytest.mark.parametrize("n", [8193, 3 * 8192 + 77, 65539])
@pytest.mark.parametrize("name,kind", SKEWED)
def test_sort_on_skewed_digits(name, kind, n):
    x = _skewed(name, n, kind)
    assert x.dtype == (np.float32 if kind == "f32" else np.float64) and np.isfinite(x).all()
    if name == "low_byte":
        assert len(np.unique(x)) == 256
    if name == "high_byte":
        assert len(np.unique(x)) == (30 if kind == "f32" else 254)
    s, _, _ = _hook(x, scan=False)
    assert np.array_equal(_bits(s), _bits(Z.java_sort(x.astype(np.float64))))


# ---- 6. the size thresholds above 2^22 ----
def test_search_above_2_23():
    """h = 4,196,353 pairs in round 1: k_zip_cnt / k_zip_compact run 2,050 workgroups, and the scan of
    their counts takes a second level."""
    n = (1 << 23) + 4099
    h, sp, got, z, pl = _full_search(_gauss(n, "f32"), 256)
    assert (z.bin_num, z.rounds) == (255, 24)  # the restatement's own figures on this input


def test_sort_and_scan_above_2_27():
    """16,386 sort tiles, 4,194,816 digit counts: the integer scan's third level.  Built and compared
    on the device.  The sorted copy is (j >> 14) - 4096: runs of 16,384 equal integers of magnitude
    up to 4,096, so every partial sum of the values (< 2^39) and of the squares (< 2^51) is an integer
    below 2^53, the int64 sums convert to double exactly and every correct order gives these doubles.
    A context of its own, its workspace released at the end."""
    from sketchml_amd.context import Context
    L = _L()
    n = (1 << 27) + 8193
    ctx = Context(torch.cuda.current_device())
    try:
        e = (torch.arange(n, dtype=torch.int64, device="cuda") >> 14) - 4096
        assert int(e[0]) == -4096 and int(e[-1]) == 4096
        gen = torch.Generator(device="cuda").manual_seed(n)
        x = e.to(torch.float32)[torch.randperm(n, device="cuda", generator=gen)]
        s, r, t = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3))
        st = L.lib.skml_debug_zip_prefix_f32(ctx.handle, _ptr(x), n, _ptr(s), _ptr(r), _ptr(t))
        assert st == 0, f"status {st}: {L.last_error()}"
        torch.cuda.synchronize()
        del x
        assert torch.equal(s.view(torch.int64), e.to(torch.float64).view(torch.int64))
        del s
        assert torch.equal(r.view(torch.int64), torch.cumsum(e, 0).to(torch.float64).view(torch.int64))
        del r
        assert torch.equal(t.view(torch.int64), torch.cumsum(e * e, 0).to(torch.float64).view(torch.int64))
    finally:
        assert L.lib.skml_zip_release_workspace(ctx.handle) == 0
        e = x = s = r = t = None
        del ctx
        torch.cuda.empty_cache()
