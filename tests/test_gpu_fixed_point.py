"""FixedPointGradient on the device against tests/fixed_point_ref.py (the numpy restatement of
ml/gradient/FixedPointGradient.scala:39-75 and BinaryUtils.java:6-29).

The device's sum of squares is a fixed tree, the reference's a sequential loop, so the two norms
differ in the last bits; the norm has a test of its own (2^-40 relative, see test_norm), and the
codes are recomputed in numpy with the norm the header holds.  Everything else is bit for bit.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import fixed_point_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 65539, (1 << 20) + 1]  # word, round / tile and multi-workgroup edges
WIDTHS = [2, 3, 7, 8, 13, 16, 29]                                 # 3, 7, 13, 29 straddle words
NP_DT = {"f32": np.float32, "f64": np.float64}


def _L():
    from sketchml_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _values(kind, n, tag=0):
    """N(0, 1) * 1e-3 in the input's dtype; read-only, shared."""
    rng = np.random.default_rng(1000 * tag + n + (7 if kind == "f64" else 0))
    v = (rng.standard_normal(n) * 1e-3).astype(NP_DT[kind])
    v.setflags(write=False)
    return v


def _dev(v):
    return torch.from_numpy(np.array(v)).cuda()


def _parse(payload, n, bits):
    """(header, words) of a payload's bytes on the host; the padding must be zero."""
    b = payload.cpu().numpy()
    h = _L().FixedHeader.from_buffer_copy(b[:64].tobytes())
    assert h.magic == _L().SKML_FIXED_MAGIC and h.n == n and h.num_bits == bits and h.words_offset == 256
    nwords = (n * bits + 63) // 64
    assert len(b) >= 256 + (nwords * 8 + 255) // 256 * 256
    assert not b[64:256].any(), "header padding"
    assert not b[256 + nwords * 8: 256 + (nwords * 8 + 255) // 256 * 256].any(), "word padding"
    return h, np.frombuffer(b[256: 256 + 8 * nwords].tobytes(), dtype="<u8")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check_encode(sk, v, bits, seed):
    """Encode v; header, codes and every word against the ref computed with the header's norm.
    Returns (payload, header, the ref's codes)."""
    n = len(v)
    pl = sk.fixed_point.encode(_dev(v), bits, seed)
    got_codes = sk.fixed_point.codes(pl, n).cpu().numpy()
    h, words = _parse(pl, n, bits)
    assert h.status == 0 and h.seed == seed
    want = R.encode_codes(v.astype(np.float64), bits, seed, norm=h.norm)
    bad = np.nonzero(got_codes != want)[0]
    assert bad.size == 0, f"{bad.size} of {n} codes differ, first at {int(bad[0])}: {got_codes[bad[0]]} != {want[bad[0]]}"
    want_words = R.pack_words(want, bits)
    badw = np.nonzero(words != want_words)[0]
    assert badw.size == 0, f"{badw.size} of {len(words)} words differ, first at {int(badw[0])}"
    return pl, h, want


# --------------------------------------------------------------------------------------------
# codes and words
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_codes_and_words(gpu, n, bits):
    for kind in ("f32", "f64"):
        for seed in (0, 11):
            _check_encode(gpu, _values(kind, n), bits, seed)


def test_worked_examples(gpu):
    sk = gpu
    v = np.array([3.0, -4.0, 0.0, 12.0, -0.0, -13.0])
    for dt in (np.float32, np.float64):
        pl = sk.fixed_point.encode(_dev(v.astype(dt)), 4, 0)
        h, words = _parse(pl, 6, 4)
        assert h.norm == math.sqrt(338.0)
        assert sk.fixed_point.codes(pl, 6).cpu().tolist() == [2, 10, 0, 5, 1, 12]
        assert words.tolist() == [0x38A054]
        pl = sk.fixed_point.encode(_dev(np.array([5.0], dtype=dt)), 4, 0)
        h, words = _parse(pl, 1, 4)
        assert h.norm == 5.0 and words.tolist() == [0x1]
        d = sk.fixed_point.decode(pl, 1, torch.float64).cpu().numpy()
        assert d[0] == 0.0 and np.signbit(d[0])
        f = sk.fixed_point.decode(pl, 1, torch.float32).cpu().numpy()
        assert f[0] == 0.0 and np.signbit(f[0])


# --------------------------------------------------------------------------------------------
# norm
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 65, 4097, 65539, (1 << 20) + 1, (1 << 22) + 4099])
def test_norm(gpu, kind, n):
    """|norm - sqrt(fsum(v^2))| <= 2^-40 norm.  The device adds the squares in a fixed tree whose
    longest chain of additions is far below 4,096; every term is >= 0, so the sum's relative error
    is below 4,097 * 2^-53 < 2^-40, the square root halves it and adds one rounding.  The squares
    themselves are exact: fp32 values have 24 significant bits, and the fp64 case uses fp32-valued
    doubles (<= 26 bits), so v * v fits a double."""
    v = _values("f32", n, tag=3).astype(NP_DT[kind])
    pl = gpu.fixed_point.encode(_dev(v), 8, 0)
    h = gpu.fixed_point.info(pl)
    want = math.sqrt(math.fsum((v.astype(np.float64) ** 2).tolist()))
    err = abs(h.norm - want)
    print(f"norm {h.norm!r} fsum {want!r} relative error {err / want:.3e} (bound {2.0 ** -40:.3e})")
    assert err <= 2.0 ** -40 * want


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_encode_is_deterministic(gpu, kind):
    """Two encodes of one buffer into buffers holding different junk: identical bytes."""
    from sketchml_amd.context import alloc_aligned
    n, bits = 65539 * 3, 13
    x = _dev(_values(kind, n, tag=4))
    nb = gpu.fixed_point.payload_bytes(n, bits)
    a = alloc_aligned(nb, "cuda").fill_(0xFF)
    b = alloc_aligned(nb, "cuda").fill_(0x5A)
    gpu.fixed_point.encode(x, bits, 9, out=a)
    gpu.fixed_point.encode(x, bits, 9, out=b)
    gpu.fixed_point.encode(x, bits, 9, out=a)
    assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------
# edge inputs
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_all_zeros(gpu, kind):
    n = 4097
    v = np.zeros(n, dtype=NP_DT[kind])
    for bits in (2, 8):
        pl, h, codes = _check_encode(gpu, v, bits, 3)
        assert h.norm == 0.0 and codes.tolist() == R.sigma_stream(3, n).tolist()
        for dt in (torch.float64, torch.float32):
            d = gpu.fixed_point.decode(pl, n, dt).cpu().numpy()
            assert not _bits(d).any(), "all +0.0"


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_minus_zero_and_the_norm_alone(gpu, kind):
    """-0.0 entries get no sign bit; an element equal to the norm with sigma = 1 gives max + 1 = the
    sign bit alone, which decodes as -0.0 ([5] with a seed whose first draw is 1)."""
    assert R.sigma_stream(0, 1)[0] == 1
    pl, h, codes = _check_encode(gpu, np.array([5.0], dtype=NP_DT[kind]), 4, 0)
    assert codes.tolist() == [8] and h.norm == 5.0
    d = gpu.fixed_point.decode(pl, 1, torch.float64).cpu().numpy()
    assert _bits(d).tolist() == _bits(np.array([-0.0])).tolist()
    v = np.zeros(65, dtype=NP_DT[kind])
    v[1::3] = -0.0
    v[40] = -7.5  # the norm alone: sqrt(56.25) is exact
    for seed in (0, 1, 2, 3):
        for bits in (3, 8, 29):
            pl, h, codes = _check_encode(gpu, v, bits, seed)
            assert h.norm == 7.5
            sign = 1 << (bits - 1)
            assert all(c in (0, 1) for c in np.delete(codes, 40)), "-0.0 has no sign bit"
            assert codes[40] == (sign if R.sigma_stream(seed, 65)[40] else sign | (sign - 1))
            want = R.decode_values(codes, bits, 7.5)
            d = gpu.fixed_point.decode(pl, 65, torch.float64).cpu().numpy()
            assert np.array_equal(_bits(d), _bits(want))


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_not_finite_values_are_refused(gpu, kind, bad):
    L = _L()
    n = 4097
    for at in (0, 2048, n - 1):
        v = np.array(_values(kind, n, tag=5))
        v[at] = bad
        pl = gpu.fixed_point.encode(_dev(v), 8, 0)
        h = gpu.fixed_point.info(pl, strict=False)
        assert h.status == L.SKML_E_NAN and h.n == n
        hdr = L.FixedHeader()
        from sketchml_amd.context import get_context
        assert L.lib.skml_fixed_info(get_context().handle, C.c_void_p(pl.data_ptr()), C.byref(hdr)) == L.SKML_E_NAN
        with pytest.raises(gpu.SketchMLException):
            gpu.fixed_point.info(pl)


def test_underflowed_norm_is_refused(gpu):
    L = _L()
    pl = gpu.fixed_point.encode(_dev(np.array([1e-200, 0.0])), 8, 0)
    h = gpu.fixed_point.info(pl, strict=False)
    assert h.status == L.SKML_E_NAN and h.norm == 0.0
    # a huge fp64 value: the sum of squares overflows, the norm is not finite
    pl = gpu.fixed_point.encode(_dev(np.array([1e200, 1.0])), 8, 0)
    assert gpu.fixed_point.info(pl, strict=False).status == L.SKML_E_NAN


def test_arguments_are_refused(gpu):
    from sketchml_amd.context import alloc_aligned, get_context
    L = _L()
    h = get_context().handle
    x = torch.zeros(1024, device="cuda")
    pl = alloc_aligned(4096, "cuda")
    enc = L.lib.skml_fixed_encode_f32
    assert enc(h, C.c_void_p(x.data_ptr()), 1024, 8, 0, C.c_void_p(pl.data_ptr()), 4096) == 0
    assert enc(h, C.c_void_p(x.data_ptr()), 1024, 1, 0, C.c_void_p(pl.data_ptr()), 4096) == L.SKML_E_ARG
    assert enc(h, C.c_void_p(x.data_ptr()), 1024, 30, 0, C.c_void_p(pl.data_ptr()), 4096) == L.SKML_E_ARG
    assert enc(h, C.c_void_p(x.data_ptr()), 0, 8, 0, C.c_void_p(pl.data_ptr()), 4096) == L.SKML_E_ARG
    assert enc(h, C.c_void_p(x.data_ptr()), 1 << 31, 8, 0, C.c_void_p(pl.data_ptr()), 4096) == L.SKML_E_ARG
    assert enc(h, C.c_void_p(x.data_ptr() + 4), 1020, 8, 0, C.c_void_p(pl.data_ptr()), 4096) == L.SKML_E_ARG
    assert enc(h, C.c_void_p(x.data_ptr()), 1024, 8, 0, C.c_void_p(pl.data_ptr()), 1024) == L.SKML_E_ARG
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------
# decode, timesBy
# --------------------------------------------------------------------------------------------
def _check_decode(sk, pl, n, codes, bits, norm):
    want = R.decode_values(codes, bits, norm)
    d = sk.fixed_point.decode(pl, n, torch.float64).cpu().numpy()
    bad = np.nonzero(_bits(d) != _bits(want))[0]
    assert bad.size == 0, f"f64: {bad.size} of {n} differ, first at {int(bad[0])}"
    f = sk.fixed_point.decode(pl, n, torch.float32).cpu().numpy()
    bad = np.nonzero(_bits(f) != _bits(want.astype(np.float32)))[0]
    assert bad.size == 0, f"f32: {bad.size} of {n} differ, first at {int(bad[0])}"


@pytest.mark.parametrize("bits", [3, 8, 29])
@pytest.mark.parametrize("n", SIZES)
def test_decode(gpu, n, bits):
    for kind in ("f32", "f64"):
        pl, h, codes = _check_encode(gpu, _values(kind, n), bits, 11)
        _check_decode(gpu, pl, n, codes, bits, h.norm)


@pytest.mark.parametrize("bits", [3, 8, 29])
def test_times_by(gpu, bits):
    n = 4097
    pl, h, codes = _check_encode(gpu, _values("f32", n), bits, 2)
    gpu.fixed_point.times_by(pl, 0.125)
    h1, words1 = _parse(pl, n, bits)
    assert h1.norm == h.norm * 0.125
    gpu.fixed_point.times_by(pl, 1.0 / 3.0)
    h2, words2 = _parse(pl, n, bits)
    assert h2.norm == h.norm * 0.125 * (1.0 / 3.0)
    assert np.array_equal(words2, R.pack_words(codes, bits)), "timesBy touches the norm alone"
    _check_decode(gpu, pl, n, codes, bits, h2.norm)


# --------------------------------------------------------------------------------------------
# decode-sum
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gathered(n, bits, P):
    """P distinct payloads (seeds 5 + p) in slots `stride` apart, and the ref's decoded doubles."""
    import sketchml_amd as sk
    from sketchml_amd.context import alloc_aligned
    nb = sk.fixed_point.payload_bytes(n, bits)
    stride = nb + 256  # slots larger than the payload
    allp = alloc_aligned(stride * P, "cuda").zero_()
    vals = []
    for p in range(P):
        v = _values("f32", n, tag=20 + p)
        slot = allp[p * stride: p * stride + nb]
        sk.fixed_point.encode(_dev(v), bits, 5 + p, out=slot)
        h = sk.fixed_point.info(slot)
        vals.append(R.decode_values(R.encode_codes(v.astype(np.float64), bits, 5 + p, norm=h.norm), bits, h.norm))
    return allp, stride, vals


@pytest.mark.parametrize("bits", [3, 8])
@pytest.mark.parametrize("n", [4097, 65539])
@pytest.mark.parametrize("P", [1, 2, 8, 9])
def test_decode_sum(gpu, P, n, bits):
    from sketchml_amd.context import get_context
    allp, stride, vals = _gathered(n, bits, 9)
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    gpu.decode_sum_fixed_point(get_context().handle, allp, P, stride, n, 1.0 / P, out)
    want = R.decode_sum(vals[:P], 1.0 / P)
    got = out.cpu().numpy()
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, f"{bad.size} of {n} sums differ, first at {int(bad[0])}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def test_decode_sum_refuses_mixed_payloads(gpu):
    from sketchml_amd.context import alloc_aligned, get_context
    L = _L()
    n = 4097
    stride = gpu.fixed_point.payload_bytes(n, 8)
    allp = alloc_aligned(stride * 2, "cuda").zero_()
    x = _dev(_values("f32", n))
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    fn = L.lib.skml_fixed_decode_sum_f32
    h = get_context().handle

    def call():
        return fn(h, C.c_void_p(allp.data_ptr()), 2, stride, C.c_void_p(out.data_ptr()), n, 0.5)

    gpu.fixed_point.encode(x, 8, 0, out=allp[:stride])
    gpu.fixed_point.encode(x, 8, 1, out=allp[stride:])
    assert call() == 0
    gpu.fixed_point.encode(x, 3, 1, out=allp[stride:])      # mixed widths
    assert call() == L.SKML_E_ARG and "bits" in L.last_error()
    gpu.fixed_point.encode(x[:4096], 8, 1, out=allp[stride:])  # mixed n
    assert call() == L.SKML_E_ARG and "values" in L.last_error()
    bad = np.array(_values("f32", n))
    bad[7] = np.nan
    gpu.fixed_point.encode(_dev(bad), 8, 1, out=allp[stride:])  # a refused input
    assert call() == L.SKML_E_NAN
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------
# gradient glue
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gradient():
    dim = 3 * 65536 + 77
    rng = np.random.default_rng(77)
    x = np.where(rng.random(dim) < 0.1, rng.standard_normal(dim), 0.0)
    x.setflags(write=False)
    return dim, x


def test_gradient_from_dense(gpu):
    sk = gpu
    dim, x = _gradient()
    dense = sk.DenseDoubleGradient(dim, _dev(x))
    g = sk.FixedPointGradient(dense, 8, seed=3)
    assert g.kind() == sk.Kind.FixedPoint and g.countNNZ() == dim and g.indices is None
    norm = g.norm
    assert abs(norm - math.sqrt(math.fsum((x * x).tolist()))) <= 2.0 ** -40 * norm
    codes = R.encode_codes(x, 8, 3, norm=norm)
    want = R.decode_values(codes, 8, norm)
    got = g.toDense()
    assert got.kind() == sk.Kind.DenseDouble and got.dim == dim and got.values.dtype == torch.float64
    assert np.array_equal(_bits(got.values.cpu().numpy()), _bits(want))
    with pytest.raises(sk.SketchMLException):
        g.toSparse()
    # toAuto picks by the decoded values' nnz (every second zero decodes to norm / max: the coin flip)
    nnz = int((np.abs(want) > 1e-8).sum())
    from sketchml_amd.gradient import auto_dense
    auto = g.toAuto()
    assert auto.kind() == (sk.Kind.DenseDouble if auto_dense(nnz, dim) else sk.Kind.SparseDouble)
    if auto.kind() == sk.Kind.SparseDouble:
        keys = np.nonzero(np.abs(want) > 1e-8)[0]
        assert np.array_equal(auto.indices.cpu().numpy(), keys)
        assert np.array_equal(_bits(auto.values.cpu().numpy()), _bits(want[keys]))
    g.timesBy(0.25)
    assert g.norm == norm * 0.25
    assert np.array_equal(_bits(g.toDense().values.cpu().numpy()), _bits(R.decode_values(codes, 8, norm * 0.25)))
    # compress's switch
    c = sk.compress(dense, "fixed_point", fixedPointBitNum=8, seed=3)
    assert c.kind() == sk.Kind.FixedPoint and torch.equal(c.payload[256:], g.payload[256:])
    assert sk.compress(dense, "FixedPoint").numBits == 8  # MLConf's default
    s1 = sk.compress(dense, "sketch", quantBinNum=64, seed=2)
    s2 = sk.SketchGradient(dense, 64, seed=2)
    assert s1.kind() == sk.Kind.Sketch and np.array_equal(_bits(s1.bucketValues), _bits(s2.bucketValues))
    assert torch.equal(s1.quantizer.getBins(), s2.quantizer.getBins())


def test_gradient_from_sparse(gpu):
    sk = gpu
    dim, x = _gradient()
    sparse = sk.DenseDoubleGradient(dim, _dev(x)).toSparse()
    keys = np.nonzero(np.abs(x) > 1e-8)[0]
    assert np.array_equal(sparse.indices.cpu().numpy(), keys)
    g = sk.FixedPointGradient(sparse, 8, seed=4)
    assert g.indices is sparse.indices and g.countNNZ() == len(keys) and g.size == len(keys)
    norm = g.norm
    codes = R.encode_codes(x[keys], 8, 4, norm=norm)
    want = R.decode_values(codes, 8, norm)
    got = g.toSparse()
    assert got.kind() == sk.Kind.SparseDouble and got.dim == dim
    assert np.array_equal(got.indices.cpu().numpy(), keys)
    assert np.array_equal(_bits(got.values.cpu().numpy()), _bits(want))
    from sketchml_amd.gradient import auto_dense
    live = int((np.abs(want) > 1e-8).sum())
    assert g.toAuto().kind() == (sk.Kind.DenseDouble if auto_dense(live, dim) else sk.Kind.SparseDouble)
    s1 = sk.compress(sparse, "Sketch", seed=2, hashSeed=5)
    s2 = sk.SketchGradient(sparse, seed=2, hashSeed=5)
    assert s1.kind() == sk.Kind.Sketch and s1.countNNZ() == s2.countNNZ()
    assert np.array_equal(_bits(s1.bucketValues), _bits(s2.bucketValues))
    k1, b1 = s1.sketch.restore_bins()
    k2, b2 = s2.sketch.restore_bins()
    assert torch.equal(k1, k2) and torch.equal(b1, b2)


# --------------------------------------------------------------------------------------------
# stream order: pattern A of tests/test_gpu_stream_order.py
# --------------------------------------------------------------------------------------------
from tests.test_gpu_stream_order import run_a, sl  # noqa: E402,F401  (sl: the calibrated delay fixture)


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_stream_order_encode_decode_sum_chain(gpu, sl, kind):  # noqa: F811
    """Two encodes, a decode and a decode-sum back to back on a non-blocking stream whose input is
    produced behind the delay: work not ordered after the stream reads the stale input (another
    dataset, another norm), work not joined back is missed by the clones."""
    from sketchml_amd.context import alloc_aligned
    L = _L()
    n, bits = 3 * 4096 + 1000, 13
    fresh_h, stale_h = _values(kind, n, tag=30), np.array(_values(kind, n, tag=31)) * 3.0 + NP_DT[kind](1e-3)
    x, fresh = _dev(stale_h), _dev(fresh_h)
    nb = gpu.fixed_point.payload_bytes(n, bits)
    allp = alloc_aligned(2 * nb, "cuda").zero_()
    dec = torch.zeros(n, dtype=torch.float64, device="cuda")
    tot = torch.zeros(n, dtype=torch.float32, device="cuda")
    enc = "skml_fixed_encode_f64" if kind == "f64" else "skml_fixed_encode_f32"

    def call(h):
        for p in range(2):
            sl.c(enc, h, C.c_void_p(x.data_ptr()), n, bits, 5 + p, C.c_void_p(allp.data_ptr() + p * nb), nb)
        sl.c("skml_fixed_decode_f64", h, C.c_void_p(allp.data_ptr()), C.c_void_p(dec.data_ptr()), n)
        sl.c("skml_fixed_decode_sum_f32", h, C.c_void_p(allp.data_ptr()), 2, nb, C.c_void_p(tot.data_ptr()), n, 0.5)

    # the decode-sum reads the headers back first, so the chain synchronises the host
    g_all, g_dec, g_tot = run_a(sl, [(x, fresh)], call, lambda: [allp, dec, tot], scribble=[allp, dec, tot], host_sync=True)
    fv = fresh_h.astype(np.float64)
    want_norm = math.sqrt(math.fsum((fv * fv).tolist()))
    vals = []
    for p in range(2):
        h, words = _parse(g_all[p * nb: (p + 1) * nb], n, bits)
        assert h.status == 0 and abs(h.norm - want_norm) <= 2.0 ** -40 * want_norm, "the norm of the stale input?"
        codes = R.encode_codes(fv, bits, 5 + p, norm=h.norm)
        assert np.array_equal(words, R.pack_words(codes, bits))
        vals.append(R.decode_values(codes, bits, h.norm))
    assert np.array_equal(_bits(g_dec.cpu().numpy()), _bits(vals[0]))
    assert np.array_equal(_bits(g_tot.cpu().numpy()), _bits(R.decode_sum(vals, 0.5)))
