"""bf16 / fp16 at the two ends of the sparse path where a dim-sized array crosses the boundary.

Input side (skml_sparse_compact_bf16 / _f16, skml_sparse_encode_bf16 / _f16): the 16-bit buffer is
compacted as its fp32 widening would be.  The reference never goes through the library's fp32
route: torch on the CPU makes the 16-bit values and widens them, numpy compacts
(|x| > 1e-8 in double, NaN out), oracle.sparse_compress encodes.

Output side (skml_sparse_decode_sum_f32 / _bf16 / _f16): oracle_sum's double sum cast to float32 by
numpy and from there to the 16-bit type by torch on the CPU; bit patterns must be equal.  With nine
payloads the sum takes a second launch, which continues from the double accumulator: a partial sum
rounded to the narrow type in between would not give the cast of the double sum."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_sparse_exchange import _dup_payload, _gather_local, _payload, oracle_sum
from test_gpu_stream_order import (BINS, GROUPS, RATIO, ROWS, _check_restored, _check_sparse_payload,
                                   _check_sparse_stream, _sparse_payload)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sketchml_amd", "csrc")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def _const(file, name):
    src = open(os.path.join(CSRC, file)).read()
    m = re.search(r"\b" + name + r" = (\d+)\b", src)
    assert m, name
    return int(m.group(1))


T = _const("skml_sparse.h", "kCompactTile")           # k_compact's tile (CompactT<bf16_t>::kTile is this constant)
CAP = _const("skml_sparse_compact.hip", "kCbCap")     # values a k_compact_big tile stages in LDS
BIG = 65536                                            # k_compact_big's tile


# --------------------------------------------------------------------------------------------
# input side
# --------------------------------------------------------------------------------------------
def _bits16(kind, dim, density, seed, special=True):
    """int16 bit patterns of a `kind` gradient: N(0, 1) at `density` rounded by torch on the CPU,
    zeros elsewhere, with +-0, NaN, +-inf and the keep test's edge patterns scattered in."""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random(dim) < density, rng.standard_normal(dim), 0.0).astype(np.float32)
    bits = torch.from_numpy(x).to(DTYPES[kind]).view(torch.int16).numpy().copy().view(np.uint16)
    if special and dim:
        inf = 0x7F80 if kind == "bf16" else 0x7C00
        pats = [0x0000, 0x8000, inf, inf | 0x8000, inf | 1, inf | 0x8041, 0x7FFF, 0xFFFF]
        if kind == "bf16":
            pats += [0x322B, 0xB22B, 0x322C, 0xB22C, 0x0001, 0x8001, 0x0080]  # threshold neighbours, tiny values
        else:
            pats += [0x0001, 0x8001, 0x03FF, 0x0400]  # the smallest subnormal (5.96e-8 > 1e-8), the largest, the first normal
        n = min(dim, max(len(pats), dim // 50))
        at = rng.choice(dim, n, replace=False)
        bits[at] = np.array(pats, dtype=np.uint16)[np.arange(n) % len(pats)]
    return bits


def _widen(kind, bits):
    """The 16-bit patterns widened to float32 by torch on the CPU."""
    return torch.from_numpy(bits.view(np.int16).copy()).view(DTYPES[kind]).float().numpy()


def _reference(kind, bits):
    w = _widen(kind, bits)
    keep = np.abs(w.astype(np.float64)) > 1e-8  # NaN compares false
    keys = np.nonzero(keep)[0].astype(np.int32)
    return keys, w[keys]


def _device16(bits, offset=0):
    """The patterns on the device, `offset` elements past a 16-byte boundary."""
    buf = torch.zeros(len(bits) + 16, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + len(bits)]
    view.copy_(torch.from_numpy(bits.view(np.int16).copy()))
    assert view.data_ptr() % 16 == (2 * offset) % 16
    return view


def _compact(gpu, kind, dev16, dim):
    from sketchml_amd import _lib
    keys = torch.full((max(dim, 1),), -1, dtype=torch.int32, device="cuda")
    vals = torch.zeros(max(dim, 1), dtype=torch.float32, device="cuda")
    nnz = C.c_int64(-1)
    fn = getattr(_lib.lib, "skml_sparse_compact_" + kind)
    st = fn(gpu.get_context().handle, C.c_void_p(dev16.data_ptr() if dim else 0), dim, C.c_void_p(keys.data_ptr()),
            C.c_void_p(vals.data_ptr()), C.byref(nnz))
    assert st == 0, _lib.last_error()
    return keys.cpu().numpy(), vals.cpu().numpy(), nnz.value


def _assert_compaction(gpu, kind, bits, offset=0):
    dim = len(bits)
    wk, wv = _reference(kind, bits)
    k, v, nnz = _compact(gpu, kind, _device16(bits, offset), dim)
    assert nnz == len(wk), (dim, nnz, len(wk))
    assert np.array_equal(k[:nnz], wk)
    assert np.array_equal(v[:nnz].view(np.uint32), wv.view(np.uint32))


SIZES = [0, 1, 7, 8, 9, T - 1, T, T + 1, 65535, 65536, 65537, 3 * 65536 + 5]


@pytest.mark.parametrize("dim", SIZES)
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_compaction_sizes_and_densities(gpu, kind, dim):
    """Keys, fp32 value bits and nnz at every size where the kernels change path (the 8-value load,
    k_compact's tile, k_compact_big's tile and a partial last tile), at densities 0, 0.1, 0.5 and 1:
    the last two keep more than kCbCap values of a 65,536-value tile, which re-reads its input."""
    for density in (0.0, 0.1, 0.5, 1.0):
        _assert_compaction(gpu, kind, _bits16(kind, dim, density, 1000 + dim))


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_compaction_at_the_stage_capacity(gpu, kind, extra):
    """One 65,536-value tile keeping exactly kCbCap values (staged in LDS) and kCbCap + 1 (re-read)."""
    rng = np.random.default_rng(7 + extra)
    x = np.zeros(BIG, dtype=np.float32)
    at = rng.choice(BIG, CAP + extra, replace=False)
    x[at] = rng.standard_normal(len(at)).astype(np.float32) + np.where(rng.random(len(at)) < 0.5, 3.0, -3.0)
    bits = torch.from_numpy(x).to(DTYPES[kind]).view(torch.int16).numpy().copy().view(np.uint16)
    assert len(_reference(kind, bits)[0]) == CAP + extra
    _assert_compaction(gpu, kind, bits)


@pytest.mark.parametrize("dim", [T + 1, 65537])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_compaction_of_a_2_byte_aligned_buffer(gpu, kind, dim):
    for density in (0.1, 1.0):
        _assert_compaction(gpu, kind, _bits16(kind, dim, density, 2000 + dim), offset=1)


def test_special_values_and_threshold_neighbours(gpu):
    """bf16 0x322B / 0xB22B (the largest magnitudes not above 1e-8) are dropped and 0x322C / 0xB22C
    kept; fp16's smallest subnormal is kept; +-0 and NaN are dropped and +-inf kept in both."""
    b = np.array([0x322B, 0xB22B, 0x322C, 0xB22C, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFF81, 0x3F80], dtype=np.uint16)
    k, v, nnz = _compact(gpu, "bf16", _device16(b), len(b))
    assert nnz == 5 and list(k[:5]) == [2, 3, 6, 7, 10]
    assert list(v[:5].view(np.uint32)) == [0x322C0000, 0xB22C0000, 0x7F800000, 0xFF800000, 0x3F800000]
    h = np.array([0x0001, 0x8001, 0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFC01, 0x3C00], dtype=np.uint16)
    k, v, nnz = _compact(gpu, "f16", _device16(h), len(h))
    assert nnz == 5 and list(k[:5]) == [0, 1, 4, 5, 8]
    assert list(v[:5].view(np.uint32)) == [0x33800000, 0xB3800000, 0x7F800000, 0xFF800000, 0x3F800000]
    _assert_compaction(gpu, "bf16", b)
    _assert_compaction(gpu, "f16", h)


def _encode(gpu, name, dev, dim, p):
    from sketchml_amd import _lib
    out = C.c_void_p()
    st = getattr(_lib.lib, name)(gpu.get_context().handle, C.c_void_p(dev.data_ptr()), dim, C.byref(p), C.byref(out))
    assert st == 0, _lib.last_error()
    return _sparse_payload(out)


@pytest.mark.parametrize("dim,density", [(300000, 0.1), (65537, 0.5)])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_encode_matches_the_oracle(gpu, kind, dim, density):
    """skml_sparse_encode_bf16 / _f16: quantizer, group tables, key streams, restore() and the
    writeObject stream equal oracle.sparse_compress of the numpy compaction; the exported blob is
    byte for byte the one skml_sparse_encode_f32 gives on the widened buffer."""
    from sketchml_amd.sparse import _params
    bits = _bits16(kind, dim, density, 3000 + dim, special=False)  # finite values: the quantizer refuses NaN
    keys, vals = _reference(kind, bits)
    osp = O.sparse_compress(keys, vals.astype(np.float64), BINS, GROUPS, ROWS, RATIO, 4, 9)
    p = _params(BINS, GROUPS, ROWS, RATIO, 4, 9)
    pl = _encode(gpu, "skml_sparse_encode_" + kind, _device16(bits), dim, p)
    assert pl.nnz() == len(keys)
    _check_sparse_payload(pl, osp)
    rk, rv = pl.restore()
    _check_restored(rk, rv, osp, len(keys))
    _check_sparse_stream(pl.serialize(), osp)
    wide = torch.from_numpy(_widen(kind, bits)).cuda()
    pl32 = _encode(gpu, "skml_sparse_encode_f32", wide, dim, p)
    from sketchml_amd.context import alloc_aligned
    assert pl.export_bytes() == pl32.export_bytes()
    # export writes the blob's sections; the padding between them is the destination's own
    blobs = [q.export(alloc_aligned(q.export_bytes(), "cuda").zero_()) for q in (pl, pl32)]
    assert torch.equal(blobs[0], blobs[1])


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_python_wrappers_take_16_bit_tensors(gpu, kind):
    dim = 65537
    bits = _bits16(kind, dim, 0.1, 4000, special=False)
    wk, wv = _reference(kind, bits)
    x16 = torch.from_numpy(bits.view(np.int16).copy()).view(DTYPES[kind])
    for x in (x16, x16.cuda()):
        k, v = gpu.to_sparse(x)
        assert v.dtype == torch.float32 and k.dtype == torch.int32
        assert np.array_equal(k.cpu().numpy(), wk)
        assert np.array_equal(v.cpu().numpy().view(np.uint32), wv.view(np.uint32))
    osp = O.sparse_compress(wk, wv.astype(np.float64), BINS, GROUPS, ROWS, RATIO, 4, 9)
    pl = gpu.encode_dense_as_sparse(x16.cuda(), BINS, GROUPS, ROWS, RATIO, 4, 9)
    _check_sparse_payload(pl, osp)
    rk, rv = pl.restore()
    _check_restored(rk, rv, osp, len(wk))
    # float32 and float64 tensors still take their own entries
    w = torch.from_numpy(_widen(kind, bits))
    k, v = gpu.to_sparse(w)
    assert v.dtype == torch.float32 and np.array_equal(v.cpu().numpy().view(np.uint32), wv.view(np.uint32))
    k, v = gpu.to_sparse(w.double())
    assert v.dtype == torch.float64 and np.array_equal(k.cpu().numpy(), wk)
    assert np.array_equal(v.cpu().numpy(), wv.astype(np.float64))


# --------------------------------------------------------------------------------------------
# output side
# --------------------------------------------------------------------------------------------
OUT_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _cast(want64, out):
    """The double sum as the entry returns it: float32 by numpy, then the 16-bit type by torch on
    the CPU; as unsigned bit patterns."""
    f = want64.astype(np.float32)
    if out == "f32":
        return f.view(np.uint32)
    return torch.from_numpy(f).to(OUT_DTYPES[out]).view(torch.int16).numpy().view(np.uint16)


def _pattern(t):
    t = t.cpu()
    return t.numpy().view(np.uint32) if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


# the shapes: payloads and the oracle's double sums (scale 1 and 1/P), built once and left unchanged
SHAPES = {
    "dense_forms": lambda gpu: [_payload(gpu, 30011, 0.97, 21, tiny=0.15), _payload(gpu, 30011, 0.3, 22, tiny=0.5),
                                _payload(gpu, 30011, 0.95, 23, tiny=0.12)],
    "eight": lambda gpu: [_payload(gpu, 2**20 + 5, 0.1 + 0.02 * p, 10 + p) for p in range(8)],
    "nine": lambda gpu: [_payload(gpu, 200003, 0.05 + 0.01 * p, 50 + p) for p in range(9)],
    "twelve_groups": lambda gpu: [_payload(gpu, 200003, 0.4, 60 + p, groups=12) for p in range(3)],
    "mixed_bins": lambda gpu: [_payload(gpu, 150001, 0.12 + 0.03 * p, 90 + p, bins=b)
                               for p, b in enumerate([512, 256, 512, 256])],
}
DIMS = {"dense_forms": 30011, "eight": 2**20 + 5, "nine": 200003, "twelve_groups": 200003, "mixed_bins": 150001}
_CASES = {}


def _case(gpu, shape):
    if shape not in _CASES:
        pls, osps = zip(*SHAPES[shape](gpu))
        dim, P = DIMS[shape], len(pls)
        allb, stride = _gather_local(pls)
        want1, forms = oracle_sum(osps, dim)
        wantp, _ = oracle_sum(osps, dim, 1.0 / P)
        _CASES[shape] = (allb, stride, dim, P, {1.0: want1, 1.0 / P: wantp}, forms, osps)
    return _CASES[shape]


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()


@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_decode_sum_shapes(gpu, shape, out):
    allb, stride, dim, P, wants, forms, _ = _case(gpu, shape)
    if shape == "dense_forms":  # the dense form's + 0.0 turns -0.0 sums into +0.0
        assert forms == ["dense", "sparse", "dense"]
    for scale, want in wants.items():
        got = gpu.decode_sum(allb, P, stride, dim, scale, dtype=OUT_DTYPES[out])
        assert got.dtype == OUT_DTYPES[out] and got.numel() == dim
        assert np.array_equal(_pattern(got), _cast(want, out)), (shape, out, scale)


@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
def test_a_continued_sum_is_rounded_once(gpu, out):
    """Nine payloads take two launches of the wave-tile form.  The result is the cast of the whole
    double sum; rounding the first eight payloads' sum to the narrow type before the ninth is added
    gives another result on this data (checked here on the oracle's numbers), so a partial sum that
    passed through `out` could not pass."""
    allb, stride, dim, P, wants, _, osps9 = _case(gpu, "nine")
    assert P == 9
    got = gpu.decode_sum(allb, P, stride, dim, 1.0, dtype=OUT_DTYPES[out])
    assert np.array_equal(_pattern(got), _cast(wants[1.0], out))
    # the f64 entry's own result is the oracle sum this is the cast of
    got64 = gpu.decode_sum(allb, P, stride, dim, 1.0)
    assert got64.dtype == torch.float64
    assert np.array_equal(got64.cpu().numpy().view(np.uint64), wants[1.0].view(np.uint64))
    first8, _ = oracle_sum(osps9[:8], dim)
    k, b = osps9[8].restore()
    if out == "f32":
        partial = first8.astype(np.float32).astype(np.float64)
    else:
        partial = torch.from_numpy(first8.astype(np.float32)).to(OUT_DTYPES[out]).double().numpy()
    partial[k] += osps9[8].q.values()[b]
    assert not np.array_equal(_cast(partial, out), _cast(wants[1.0], out))


def _small_sum(gpu, dim, out, forms, offset=0):
    # a single value gives two bins, which calGroupEdges cannot split into 8 groups: two groups at dim 1
    pls, osps = zip(*[_payload(gpu, dim, 1.0 if dim == 1 else 0.6, 300 + dim + p, groups=2 if dim == 1 else 8)
                      for p in range(2)])
    allb, stride = _gather_local(pls)
    want, _ = oracle_sum(osps, dim, 0.5)
    from sketchml_amd import _lib
    dt = OUT_DTYPES[out]
    per = 16 // torch.empty(0, dtype=dt).element_size()
    buf = torch.zeros(dim + 2 * per, dtype=dt, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dst = buf[offset:offset + dim]
    with _lib.forced_forms(**forms):
        got = gpu.decode_sum(allb, 2, stride, dim, 0.5, out=dst)
    assert np.array_equal(_pattern(got), _cast(want, out)), (dim, out, forms, offset)
    rest = torch.cat([buf[:offset], buf[offset + dim:]]).float()
    assert not (rest != 0).any()  # nothing written outside out[0, dim)


@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
def test_decode_sum_tile_edges(gpu, out):
    """One key below, at and above a tile of the wave-tile form (512 keys) and of the 4,096-key
    tiles: the last partial tile takes element stores, a whole one 16-byte stores."""
    for dim in (1, 511, 512, 513):
        _small_sum(gpu, dim, out, {})
    for dim in (4095, 4096, 4097):
        _small_sum(gpu, dim, out, {"agg_tiles": 1})


@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
def test_decode_sum_into_an_unaligned_out(gpu, out):
    """`out` one element past a 16-byte boundary: element stores throughout."""
    _small_sum(gpu, 513, out, {}, offset=1)
    _small_sum(gpu, 4097, out, {"agg_tiles": 1}, offset=1)


@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
def test_decode_sum_refusals(gpu, out):
    """A key repeated across a payload's groups and an empty payload raise the f64 entry's messages;
    the next good call on the same context is exact."""
    dim = 100003
    good = [_payload(gpu, dim, 0.2, 71)]
    p1, o1 = _dup_payload(gpu, dim, 72)
    pls = [good[0][0], p1]
    allb, stride = _gather_local(pls)
    dt = OUT_DTYPES[out]
    with pytest.raises(gpu.SketchMLException, match="strictly increasing"):
        gpu.decode_sum(allb, 2, stride, dim, dtype=dt)
    empty = gpu.encode_sparse(torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.float64).cuda())
    for order in ([empty, good[0][0]], [good[0][0], empty]):
        eb, es = _gather_local(order)
        with pytest.raises(gpu.SketchMLException, match="head of empty list"):
            gpu.decode_sum(eb, 2, es, dim, dtype=dt)
    allb, stride = _gather_local(pls[:1])
    got = gpu.decode_sum(allb, 1, stride, dim, dtype=dt)
    want, _ = oracle_sum([good[0][1]], dim)
    assert np.array_equal(_pattern(got), _cast(want, out))


def test_decode_sum_dtype_dispatch(gpu):
    dim = 30011
    pl, osp = _payload(gpu, dim, 0.3, 22)
    allb, stride = _gather_local([pl])
    with pytest.raises(gpu.SketchMLException, match="dtype"):
        gpu.decode_sum(allb, 1, stride, dim, dtype=torch.int32)
    with pytest.raises(gpu.SketchMLException, match="dtype"):
        gpu.decode_sum(allb, 1, stride, dim, out=torch.zeros(dim, dtype=torch.int32, device="cuda"))
    want, _ = oracle_sum([osp], dim)
    got = gpu.decode_sum(allb, 1, stride, dim)
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
    dst = torch.zeros(dim, dtype=torch.bfloat16, device="cuda")
    got = gpu.decode_sum(allb, 1, stride, dim, out=dst)  # out's dtype decides
    assert got.data_ptr() == dst.data_ptr() and np.array_equal(_pattern(got), _cast(want, "bf16"))


def test_exchange_sparse_out_dtype_world1(gpu):
    import torch.distributed as dist
    from sketchml_amd import distributed as D
    store = dist.HashStore()
    dist.init_process_group("gloo", store=store, rank=0, world_size=1)
    try:
        dim = 100003
        pl, osp = _payload(gpu, dim, 0.1, 41)
        ex = D.PayloadExchange(gpu.get_context().handle)
        try:
            avg, allb, stride = D.exchange_sparse(pl, dim, exchange=ex, out_dtype=torch.bfloat16)
            avg64, _, _ = D.exchange_sparse(pl, dim, exchange=ex)
            torch.cuda.synchronize()
        finally:
            ex.close()
        want, _ = oracle_sum([osp], dim)
        assert avg.dtype == torch.bfloat16 and np.array_equal(_pattern(avg), _cast(want, "bf16"))
        assert avg64.dtype == torch.float64 and np.array_equal(avg64.cpu().numpy().view(np.uint64), want.view(np.uint64))
    finally:
        dist.destroy_process_group()
