"""bf16 / fp16 gradients through the dense codec without an fp32 copy, against the CPU oracle.

A 16-bit encode is defined as the fp32 encode of the widened buffer (widening is exact), so the
reference is oracle.quantize of the widened values as doubles: binNum, zeroIdx, min, max and every
split equal, bins bit-exact, decoded fp32 equal.  A 16-bit decode / decode-sum is the oracle's fp32
result rounded to the 16-bit type by torch on the CPU (round to nearest even), compared bit for
bit.  The library's own fp32 path is never the reference; one extra assertion checks that the
payload of quantize(x16) is byte-identical to that of quantize(x16.float()).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
ENCODE = {"bf16": "skml_dense_encode_bf16", "fp16": "skml_dense_encode_f16"}
DECODE = {"bf16": "skml_dense_decode_bf16", "fp16": "skml_dense_decode_f16"}


@pytest.fixture(params=list(DTYPES))
def dt(request):
    return request.param


def _data(n, seed, kind, dt):
    """fp32 data on the CPU, rounded to the 16-bit type by torch on the CPU: (x16, widened fp32)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "normal":
        pass
    elif kind == "signed_zero":  # hands the leaf over to its exact loop
        r = rng.random(n)
        x[r < 0.2] = 0.0
        x[(r >= 0.2) & (r < 0.4)] = -0.0
    elif kind == "dups":
        x = rng.integers(-5, 6, n).astype(np.float32)
    elif kind == "const":
        x = np.full(n, 3.25, dtype=np.float32)
    elif kind == "special":  # +-inf and subnormals of the 16-bit type
        subs = (6e-8, -6e-8, 3e-6, -3e-6) if dt == "fp16" else (1e-40, -1e-40)
        for s in subs:
            x[rng.random(n) < 0.04] = np.float32(s)
        x[rng.random(n) < 0.01] = np.inf
        x[rng.random(n) < 0.01] = -np.inf
    else:
        raise ValueError(kind)
    x16 = torch.from_numpy(x).to(DTYPES[dt])
    wide = x16.float().numpy()
    if kind == "special":  # the subnormals survived the rounding as subnormals of the type
        tiny = np.abs(wide[(wide != 0) & np.isfinite(wide)]).min()
        assert tiny < (6.2e-5 if dt == "fp16" else 1.2e-38)
    return x16, wide


@functools.lru_cache(maxsize=None)
def _case(dt, n, kind, bins, seed, dedup=True):
    """Input and oracle result of one encode, computed once and shared (never modified)."""
    x16, wide = _data(n, 31 * n + seed, kind, dt)
    xd = wide.astype(np.float64)
    oq = O.quantize(xd, bins, seed) if dedup else O.parallel_quantize(xd, bins, threads=1, seed=seed)
    return x16, wide, oq


def _check(gq, oq):
    assert gq.getBinNum() == oq.bin_num
    assert gq.getZeroIdx() == oq.zero_idx
    assert gq.getMin() == oq.min and gq.getMax() == oq.max
    gs = gq.getSplits()
    assert gs.shape == oq.splits.shape
    assert np.array_equal(gs.view(np.uint64), oq.splits.view(np.uint64)) or np.array_equal(gs, oq.splits)
    assert np.array_equal(gq.getBins().cpu().numpy(), oq.bins)
    dec = gq.decode()
    assert dec.dtype == torch.float32  # the default decode dtype stays fp32 for 16-bit input
    want = oq.values()[oq.bins].astype(np.float32)
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), want.view(np.uint32))


def _live_bytes(q):
    """Header, live splits and the n codes of a payload (not the alignment padding)."""
    h = q._load_header()
    pl = q.payload.cpu()
    return torch.cat([pl[:64 + 8 * (h.bin_num - 1)], pl[h.codes_offset:h.codes_offset + (q.n * h.code_bits + 7) // 8]])


def _same16(got, want):
    """Bit patterns equal; a position where both sides are NaN counts as equal."""
    g, w = got.cpu(), want.cpu()
    assert g.dtype == w.dtype and g.shape == w.shape
    ok = (g.view(torch.int16) == w.view(torch.int16)) | (torch.isnan(g) & torch.isnan(w))
    assert bool(ok.all()), f"{int((~ok).sum())} of {ok.numel()} differ, first at {int((~ok).nonzero()[0])}"


def _params(bins, seed, dedup=1):
    from sketchml_amd import _lib
    p = _lib.Params()
    _lib.lib.skml_params_default(C.byref(p))
    p.bin_num, p.seed, p.dedup = bins, seed, dedup
    return p


def _raw_encode(gpu, dt, x, bins, seed, dedup):
    """The C entry itself; returns (status, a Quantizer over the payload)."""
    from sketchml_amd import _lib
    n = x.numel()
    q = gpu.QuantileQuantizer(bins, seed)
    nb = _lib.lib.skml_dense_payload_bytes(n, bins)
    q.payload, q.n, q.device = gpu.alloc_aligned(nb, x.device), n, x.device
    st = getattr(_lib.lib, ENCODE[dt])(gpu.get_context(x.device).handle, C.c_void_p(x.data_ptr()), n,
                                       C.byref(_params(bins, seed, dedup)), C.c_void_p(q.payload.data_ptr()), nb)
    return st, q


# ---- 1. encode parity ------------------------------------------------------------------------
# no chunk / one chunk / tail only; the quantize tile and its tail; exactly one 64-chunk leaf tile;
# a full tile + a partial tile + a base-buffer tail; several tiles, merge passes, split leaf forms
SIZES = [1, 255, 256, 257, 1000, 1024, 1025, 16384, 16384 + 300, 65536 * 2 + 777, 2**20 + 12345]


@pytest.mark.parametrize("n", SIZES)
def test_encode_sizes(gpu, dt, n):
    seed = 1000 + n
    x16, _, oq = _case(dt, n, "normal", 256, seed)
    x = x16.cuda()
    gq = gpu.QuantileQuantizer(256, seed=seed)
    gq.quantize(x)
    _check(gq, oq)
    g32 = gpu.QuantileQuantizer(256, seed=seed)
    g32.quantize(x.float())
    assert torch.equal(_live_bytes(gq), _live_bytes(g32))  # the input type does not reach the payload


@pytest.mark.parametrize("kind", ["normal", "signed_zero", "dups", "const", "special"])
@pytest.mark.parametrize("n", [300, 4096 * 3 + 11, 2**18 + 5])
def test_encode_edge_data(gpu, dt, kind, n):
    x16, _, oq = _case(dt, n, kind, 256, 77)
    gq = gpu.QuantileQuantizer(256, seed=77)
    gq.quantize(x16.cuda())
    _check(gq, oq)


def test_encode_no_dedup_through_the_c_entry(gpu, dt):
    x16, _, oq = _case(dt, 70000, "dups", 64, 5, dedup=False)
    st, q = _raw_encode(gpu, dt, x16.cuda(), 64, 5, dedup=0)
    assert st == 0
    assert q.getBinNum() == 64  # duplicate splits kept
    _check(q, oq)


@pytest.mark.parametrize("bins", [2, 16, 256, 1000])  # code widths 1, 4, 8, 16
def test_encode_code_widths(gpu, dt, bins):
    n = 3 * 2**16 + 999
    x16, _, oq = _case(dt, n, "normal", bins, bins)
    gq = gpu.QuantileQuantizer(bins, seed=bins)
    gq.quantize(x16.cuda())
    assert gq.codeBits() == {2: 1, 16: 4, 256: 8, 1000: 16}[bins] or gq.getBinNum() < bins
    _check(gq, oq)


def test_encode_wide_split_table(gpu, dt):
    """5,000 splits kept (dedup = 0): the quantize pass searches the payload's splits and the
    16-bit decode computes the midpoints from them (no LDS table)."""
    n = 16384 + 300
    x16, _, oq = _case(dt, n, "normal", 5000, 9, dedup=False)
    st, q = _raw_encode(gpu, dt, x16.cuda(), 5000, 9, dedup=0)
    assert st == 0 and q.getBinNum() == 5000
    _check(q, oq)
    want = torch.from_numpy(oq.values()[oq.bins].astype(np.float32)).to(DTYPES[dt])
    _same16(q.decode(dtype=DTYPES[dt]), want)


# ---- 2. NaN ----------------------------------------------------------------------------------
N_NAN = 16384 + 20 * 256 + 100  # a full leaf tile, a partial tile of 20 chunks, a tail of 100


@pytest.mark.parametrize("pos", [5000, 16384 + 1000, N_NAN - 3], ids=["full_tile", "partial_tile", "tail"])
def test_nan_raises(gpu, dt, pos):
    x16 = _case(dt, N_NAN, "normal", 256, 3)[0].clone()
    x16[pos] = float("nan")
    with pytest.raises(gpu.QuantileSketchException, match="NaN"):
        gpu.QuantileQuantizer(256, seed=3).quantize(x16.cuda())


# ---- 3. alignment ----------------------------------------------------------------------------
def test_alignment(gpu, dt):
    from sketchml_amd import _lib
    n = 16384 + 300
    x16, _, oq = _case(dt, n, "normal", 256, 1000 + n)
    buf = torch.empty(n + 16, dtype=DTYPES[dt], device="cuda")
    assert buf.data_ptr() % 16 == 0
    v8 = buf[8:8 + n]  # 16 bytes in: encoded in place
    v8.copy_(x16)
    q = gpu.QuantileQuantizer(256, seed=1000 + n, deferred=True)
    q.quantize(v8)
    assert q._x.data_ptr() == v8.data_ptr()
    _check(q, oq)
    v1 = buf[1:1 + n]  # 2 bytes in: Python clones it
    v1.copy_(x16)
    q = gpu.QuantileQuantizer(256, seed=1000 + n, deferred=True)
    q.quantize(v1)
    assert q._x.data_ptr() != v1.data_ptr() and q._x.data_ptr() % 16 == 0
    _check(q, oq)
    st, _ = _raw_encode(gpu, dt, v1, 256, 1, dedup=1)  # the C entry refuses the pointer
    assert st == _lib.SKML_E_ARG


# ---- 4. decode to 16 bit ---------------------------------------------------------------------
def _decode_both_alignments(gpu, q, odt, want):
    """q.decode into an aligned tensor, and the C entry into a pointer that is only 2-byte aligned."""
    from sketchml_amd import _lib
    got = q.decode(dtype=DTYPES[odt])
    assert got.dtype == DTYPES[odt]
    _same16(got, want)
    buf = torch.zeros(q.n + 9, dtype=DTYPES[odt], device="cuda")
    out = buf[1:1 + q.n]
    assert out.data_ptr() % 16 == 2
    st = getattr(_lib.lib, DECODE[odt])(gpu.get_context().handle, C.c_void_p(q.payload.data_ptr()),
                                        C.c_void_p(out.data_ptr()), q.n)
    assert st == 0, _lib.last_error()
    _same16(out, want)
    assert float(buf[0]) == 0 and not buf[1 + q.n:].any()  # nothing written around the output


@pytest.mark.parametrize("odt", list(DTYPES))
@pytest.mark.parametrize("bins", [4, 256, 5000])
@pytest.mark.parametrize("n", [1, 7, 1024, 1025, 16384 + 300])
def test_decode_to_16_bit(gpu, dt, odt, n, bins):
    seed = 1000 + n
    x16, _, oq = _case(dt, n, "normal", bins, seed)
    q = gpu.QuantileQuantizer(bins, seed=seed)
    q.quantize(x16.cuda())
    want = torch.from_numpy(oq.values()[oq.bins].astype(np.float32)).to(DTYPES[odt])
    _decode_both_alignments(gpu, q, odt, want)


@pytest.mark.parametrize("odt", list(DTYPES))
def test_decode_fp32_payload_to_16_bit(gpu, odt):
    n = 16384 + 300
    x = np.random.default_rng(12).standard_normal(n).astype(np.float32)
    oq = O.quantize(x.astype(np.float64), 256, 12)
    q = gpu.QuantileQuantizer(256, seed=12)
    q.quantize(torch.from_numpy(x).cuda())
    want = torch.from_numpy(oq.values()[oq.bins].astype(np.float32)).to(DTYPES[odt])
    _decode_both_alignments(gpu, q, odt, want)


# ---- 5. decode-sum to 16 bit -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gathered(dt, n, bins, P, dedup=True):
    """P payloads of distinct seeds laid out `stride` apart, and the oracle's decoded doubles."""
    import sketchml_amd as sk
    from sketchml_amd import _lib
    nb = _lib.lib.skml_dense_payload_bytes(n, bins)
    stride = (nb + 255) // 256 * 256
    allp = sk.alloc_aligned(stride * P, "cuda")
    decoded = []
    for r in range(P):
        x16, _, oq = _case(dt, n, "normal", bins, 4 + r, dedup)
        q = sk.QuantileQuantizer(bins, seed=4 + r)
        q._encode(x16.cuda(), dedup=dedup)
        assert q.getBinNum() == oq.bin_num
        allp[r * stride:r * stride + nb].copy_(q.payload)
        decoded.append(oq.values()[oq.bins])
    torch.cuda.synchronize()
    return allp, stride, decoded


def _check_decode_sum(gpu, dt, n, bins, P, dedup=True):
    from sketchml_amd import _lib
    from sketchml_amd import distributed as D
    allp, stride, decoded = _gathered(dt, n, bins, 8 if P <= 8 and bins == 256 else P, dedup)
    acc = np.zeros(n, dtype=np.float64)
    for r in range(P):  # payload order, in float64 (Gradient.sum)
        acc += decoded[r]
    want = torch.from_numpy((acc * (1.0 / P)).astype(np.float32)).to(DTYPES[dt])
    ctx = gpu.get_context().handle
    for form in (0, 1):  # the library's choice, and the per-payload kernel forced
        with _lib.forced_forms(decode_sum=form):
            out = torch.zeros(n, dtype=DTYPES[dt], device="cuda")
            D.decode_sum(ctx, allp, P, stride, n, 1.0 / P, out)
            _same16(out, want)
            buf = torch.zeros(n + 9, dtype=DTYPES[dt], device="cuda")  # an output 2 bytes off 16
            D.decode_sum(ctx, allp, P, stride, n, 1.0 / P, buf[1:1 + n])
            _same16(buf[1:1 + n], want)
            assert float(buf[0]) == 0 and not buf[1 + n:].any()


@pytest.mark.parametrize("n", [40005, 2**20 + 13])
@pytest.mark.parametrize("P", [1, 3, 8])
def test_decode_sum_to_16_bit(gpu, dt, P, n):
    _check_decode_sum(gpu, dt, n, 256, P)


def test_decode_sum_narrow_codes(gpu, dt):
    _check_decode_sum(gpu, dt, 40005, 4, 3)


def test_decode_sum_eight_tables_of_1024_bins(gpu, dt):
    """8 x 1,024 bins (kept by dedup = 0) do not fit the occupancy form's LDS: the per-payload
    kernel is the library's own choice."""
    _check_decode_sum(gpu, dt, 40005, 1024, 8, dedup=False)


def test_decode_sum_refuses_other_dtypes(gpu, dt):
    from sketchml_amd import distributed as D
    allp, stride, _ = _gathered(dt, 40005, 4, 3)
    with pytest.raises(gpu.SketchMLException):
        D.decode_sum(gpu.get_context().handle, allp, 3, stride, 40005, 1.0,
                     torch.empty(40005, dtype=torch.float64, device="cuda"))


# ---- 6. no silent upcast ---------------------------------------------------------------------
def test_no_silent_upcast(gpu, dt):
    n = 16384 + 300
    x16, wide, oq = _case(dt, n, "normal", 256, 1000 + n)
    q = gpu.QuantileQuantizer(256, seed=1000 + n, deferred=True)
    q.quantize(x16.cuda())
    assert q._x.dtype == DTYPES[dt]  # the encode read the 16-bit tensor itself
    _check(q, oq)
    u = gpu.UniformQuantizer(256)
    u.quantize(x16.cuda())  # no 16-bit entry: the kept fp32 upcast, same result
    _check(u, O.uniform_quantize(wide.astype(np.float64), 256))
