"""ZipMLQuantizer on the device (skml_zip_encode_*, sketchml_amd/csrc/skml_zip.hip) against the numpy
restatement tests/zipml_ref.py.

What is defined bit for bit: the sorted copy (Arrays.sort's total order), and -- given the prefix sums
-- the split search, min, max, zeroIdx and the bins.  The prefix sums themselves are a fixed tree
that rounds unlike the reference's sequential loop, so they get a bound of their own: D * 2^-53 *
sum |s_j| with D = the additions on the tree's longest path (zip_scan_depth of skml_zip.hpp, restated
here from the tree's block sizes), and exact equality where every summation order gives the same
doubles (integers with all partial sums below 2^53).

Sizes: the issue's list, plus the neighbours of the sizes at which the code changes form: 2,048 (one
workgroup of the scan tree), 4,096 (the one-workgroup tail, kZipTail), 8,192 (one sort tile) and
2^22 = 2,048^2 (above it the workgroup totals no longer fit one workgroup: a third tree level, the
totals-only pass over totals, D = 53 -- the form every size from 2^24 up runs)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import zipml_ref as Z
from tests.test_gpu_stream_order import _drain, _parse, run_a, run_b, sl  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

SIZES = [2, 5, 255, 256, 257, 258, 300, 511, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 65539,
         (1 << 20) + 1]
BIG = [(1 << 22) - 1, 1 << 22, (1 << 22) + 1]  # around the scan tree's third level
BINS = [4, 16, 256]
CASES = ([(n, b) for n in SIZES for b in BINS] + [(65539, 65536), ((1 << 20) + 1, 65536)]
         + [(n, 256) for n in BIG] + [((1 << 22) + 1, 16)])
KINDS = ["f32", "f64"]
SCAN_THREAD, SCAN_WAVE, SCAN_WAVES, SCAN_BLOCK = 8, 6, 4, 2048  # the scan tree of skml_zip.hip


def _L():
    from sketchml_amd import _lib
    return _lib


def _ctx():
    from sketchml_amd.context import get_context
    return get_context()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def scan_depth(n, d0=0):
    """Additions behind one output of the prefix-sum tree over n leaves of depth d0: a thread's 8
    values in order (7), the wave's Hillis-Steele scan (6), the offset of the last of 4 waves (2; 3
    for the workgroup total), wave offset + lane offset (1), + the thread's own prefix (1); with
    more than one workgroup the total of the workgroups before (out of the same tree over the
    workgroup totals) is added to wave + lane offset first: one addition more on either path."""
    local = d0 + (SCAN_THREAD - 1) + SCAN_WAVE + (SCAN_WAVES - 2) + 1 + 1
    if n <= SCAN_BLOCK:
        return local
    up = scan_depth(-(-n // SCAN_BLOCK), d0 + (SCAN_THREAD - 1) + SCAN_WAVE + (SCAN_WAVES - 1))
    return max(up + 2, local + 1)


def test_scan_depth_figures():
    assert [scan_depth(n) for n in (2, 2048, 2049, (1 << 20) + 1, 1 << 22, (1 << 22) + 1, 1 << 28)] == [17, 17, 35, 35, 35, 53, 53]


# ---- data, computed once and never modified ----
@functools.lru_cache(maxsize=None)
def _gauss(n, kind):
    """N(0,1) * 1e-3: the inputs the restatement was checked to terminate on."""
    x = np.random.default_rng(1000 + n).standard_normal(n) * 1e-3
    return x.astype(np.float32) if kind == "f32" else x


@functools.lru_cache(maxsize=None)
def _special(n, kind, extremes=True):
    """Signed zeros, denormals, duplicates and (extremes) +-max among gaussian values.  Without the
    extremes the largest magnitudes are +-1e150, whose squares still are finite doubles."""
    dt = np.float32 if kind == "f32" else np.float64
    x = _gauss(n, kind).copy()
    tiny = np.finfo(dt).smallest_subnormal
    big = np.finfo(dt).max if extremes else dt(min(1e150, float(np.finfo(dt).max)))
    sp = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, big, -big, np.finfo(dt).tiny, -0.0, 0.0], dtype=dt)
    k = min(n, len(sp))
    x[np.random.default_rng(n).permutation(n)[:k]] = sp[:k]
    if n >= 64:
        x[n // 2: n // 2 + 16] = x[n // 3]  # duplicates
    return x


@functools.lru_cache(maxsize=None)
def _integers(n):
    """Distinct integers from [-2^17, 2^17]: every partial sum of values (< 2^37) and squares (< 2^54 / 4)
    is an integer below 2^53, so every summation order gives the same doubles."""
    assert n <= 65539
    return np.random.default_rng(n).permutation(np.arange(-(1 << 17), (1 << 17) + 1))[:n].astype(np.float64)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _hook(x, h=None, scan=True):
    """(sorted, r, t) of the debug hook: the encode's own sort and scan."""
    L = _L()
    xd = _dev(x)
    n = xd.numel()
    s, r, t = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3))
    fn = L.lib.skml_debug_zip_prefix_f64 if xd.dtype == torch.float64 else L.lib.skml_debug_zip_prefix_f32
    st = fn(h or _ctx().handle, _ptr(xd), n, _ptr(s), _ptr(r) if scan else None, _ptr(t) if scan else None)
    assert st == 0, f"status {st}: {L.last_error()}"
    return s.cpu().numpy(), r.cpu().numpy(), t.cpu().numpy()


def _encode(x, bins, h=None, cap_delta=0):
    """(status, payload) of skml_zip_encode_* on a 0xFF-filled payload."""
    from sketchml_amd.context import alloc_aligned
    L = _L()
    xd = _dev(x)
    n = xd.numel()
    nb = L.lib.skml_dense_payload_bytes(n, bins)
    pl = alloc_aligned(max(nb, 256), "cuda").fill_(0xFF)
    fn = L.lib.skml_zip_encode_f64 if xd.dtype == torch.float64 else L.lib.skml_zip_encode_f32
    st = fn(h or _ctx().handle, _ptr(xd), n, bins, _ptr(pl), nb + cap_delta)
    torch.cuda.synchronize()
    return st, pl


def _check_search(x, bins, ref_prefix=None):
    """The payload of x against the restatement run on the hook's own sorted / r / t (or on
    ref_prefix); returns (header, splits, device bins, restatement)."""
    s, r, t = _hook(x)
    z = Z.quantize(x, bins, *(ref_prefix or (s, r, t)))
    st, pl = _encode(x, bins)
    if z.status != Z.OK:
        assert st == _L().SKML_E_ARG and "does not terminate" in _L().last_error()
        return None
    assert st == 0, f"status {st}: {_L().last_error()}"
    h, sp, got = _parse(pl)
    assert (h.n, h.bin_num, h.req_bins, h.zero_idx) == (len(x), z.bin_num, bins, z.zero_idx)
    assert np.array_equal(_bits([h.min, h.max]), _bits([z.min, z.max]))
    assert np.array_equal(_bits(sp), _bits(z.splits))
    return h, sp, got, z, pl


# ---- 1. sort ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES + BIG)
def test_sorted_copy_is_arrays_sort(n, kind):
    x = _special(n, kind)
    s, _, _ = _hook(x, scan=False)
    wide = x.astype(np.float64)
    assert np.array_equal(s, np.sort(wide))                       # the order of the values
    assert np.array_equal(_bits(s), _bits(Z.java_sort(wide)))     # and of -0.0 / +0.0, bit for bit


# ---- 2. prefix sums where every order gives the same doubles ----
@pytest.mark.parametrize("n", [n for n in SIZES if n <= 65539])
def test_prefix_sums_exact_on_integers(n):
    x = _integers(n)
    s, r, t = _hook(x)
    ss = np.sort(x)
    assert np.array_equal(_bits(s), _bits(ss))
    assert np.array_equal(_bits(r), _bits(np.cumsum(ss))) and np.array_equal(_bits(t), _bits(np.cumsum(ss * ss)))
    xf = x.astype(np.float32)  # the fp32 entry widens after the sort
    s, r, t = _hook(xf)
    assert np.array_equal(_bits(r), _bits(np.cumsum(ss))) and np.array_equal(_bits(t), _bits(np.cumsum(ss * ss)))


# ---- 3. prefix sums in general: the tree's bound against exact integer sums ----
def _as_ints(a, e0):
    """The doubles as Python integers in units of 2^e0 (every value a multiple of it)."""
    m, e = np.frexp(a)
    mi = (m * float(1 << 53)).astype(np.int64).astype(object)
    sh = np.where(a == 0, 0, e.astype(np.int64) - 53 - e0)
    assert sh.min() >= 0
    return mi << sh.astype(object)


@pytest.mark.parametrize("n,kind", [(n, k) for n in SIZES for k in KINDS] + [(n, "f32") for n in BIG])
def test_prefix_sums_within_the_tree_bound(n, kind):
    x = _gauss(n, kind)
    s, r, t = _hook(x)
    D = scan_depth(n)
    nz = s[s != 0]
    e0 = int(np.frexp(np.abs(nz).min())[1]) - 53 - 53  # a rounded sum of multiples of 2^e is one too
    si = _as_ints(s, e0)
    exact, mass = np.cumsum(si), np.cumsum(np.abs(si))
    err = np.abs(_as_ints(r, e0) - exact)
    bad = np.nonzero((err << 53) > D * mass)[0]
    assert not len(bad), f"r: {len(bad)} of {n} outside D = {D}, first {bad[0]}"
    # t: the squares are rounded once more, exact squares in units of 2^(2 e0)
    sq = si * si
    exact2 = np.cumsum(sq)
    err2 = np.abs(_as_ints(t, 2 * e0) - exact2)
    bad = np.nonzero((err2 << 53) > (D + 1) * exact2)[0]
    assert not len(bad), f"t: {len(bad)} of {n} outside D + 1 = {D + 1}, first {bad[0]}"


# ---- 4 + 5. the split search and the bins ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,bins", CASES)
def test_split_search_and_bins(n, bins, kind):
    L = _L()
    x = _gauss(n, kind)
    res = _check_search(x, bins)
    assert res is not None, "the restatement terminates on these inputs"
    h, sp, got, z, pl = res
    # B or B - 1 as a rule; fewer when rounding left some errors below the zeros that pad the select
    assert 2 <= z.bin_num <= min(n, bins) and z.rounds == L.lib.skml_debug_zip_rounds(_ctx().handle)
    assert np.array_equal(got, z.bins(x))
    if kind == "f32":
        # byte for byte the codes of the split-injected encode with the header's splits, min and max
        from sketchml_amd.context import alloc_aligned
        nb = L.lib.skml_dense_payload_bytes(n, h.bin_num)
        pl2 = alloc_aligned(nb, "cuda").fill_(0xFF)
        spc = np.ascontiguousarray(sp)
        xd = _dev(x)
        st = L.lib.skml_dense_encode_with_splits_f32(_ctx().handle, _ptr(xd), n, spc.ctypes.data_as(L.dblp), len(spc),
                                                     h.min, h.max, _ptr(pl2), nb)
        assert st == 0, L.last_error()
        h2, _, got2 = _parse(pl2)
        nbytes = (n * h.code_bits + 7) // 8
        a = pl.cpu().numpy()[h.codes_offset: h.codes_offset + nbytes]
        b = pl2.cpu().numpy()[h2.codes_offset: h2.codes_offset + nbytes]
        assert h.code_bits == h2.code_bits and np.array_equal(a, b) and h.zero_idx == h2.zero_idx
    else:
        # the oracle's Quantizer.indexOf on the header's table
        qh = O.QuantHeader()
        qh.bin_num, qh.n, qh.zero_idx, qh.min, qh.max = h.bin_num, n, h.zero_idx, h.min, h.max
        for i, v in enumerate(sp):
            qh.splits[i] = v
        oq = O.OracleQuant(qh, None)
        pick = np.arange(n) if n <= 4097 else np.random.default_rng(n).choice(n, 3000, replace=False)
        assert [int(got[i]) for i in pick] == [oq.index_of(float(x[i])) for i in pick]


@pytest.mark.parametrize("n", [257, 300, 4097, 65539])
def test_full_parity_on_exact_inputs(n):
    """Integers: the device's prefix sums are the sequential ones, so the payload equals the
    restatement run entirely on its own (its own sort and cumsum)."""
    x = _integers(n)
    for bins in BINS:
        s = Z.java_sort(x)
        assert _check_search(x, bins, (s, *Z.prefix_sums(s))) is not None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [258, 4097, 8193])
def test_special_values_follow_the_restatement(n, kind):
    """Zeros, denormals, duplicates and huge magnitudes: whatever the restatement says (a result, or
    a stall).  fp64 +-max is left out: its square overflows, t becomes inf and the errors NaN, and
    what the search does after that is not specified."""
    _check_search(_special(n, kind, extremes=kind == "f32"), 16)


def _same_payload(a, b):
    (ha, sa, ba), (hb, sb, bb) = _parse(a), _parse(b)
    assert bytes(ha) == bytes(hb) and np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(ba, bb)


# ---- 6. consumers ----
def test_consumers_work_on_a_zip_payload():
    import sketchml_amd as sk
    n = 65539
    x, y = _gauss(n, "f32"), _gauss(n + 1, "f32")[:n] * 2
    q = sk.ZipMLQuantizer(256)
    q.quantize(_dev(x))
    h, sp, bins = _parse(q.payload)
    z = Z.ZipResult(Z.OK, h.bin_num, sp, h.min, h.max, h.zero_idx)
    vals = z.values()
    assert np.array_equal(q.getValues(), vals) and np.array_equal(q.getSplits(), sp)
    assert np.array_equal(q.getBins().cpu().numpy(), bins) and np.array_equal(bins, z.bins(x))
    assert np.array_equal(q.decode().cpu().numpy(), vals[bins].astype(np.float32))
    assert np.array_equal(q.decode(dtype=torch.float64).cpu().numpy(), vals[bins])
    assert np.array_equal(q.decode(dtype=torch.bfloat16).float().cpu().numpy(),
                          torch.from_numpy(vals[bins].astype(np.float32)).to(torch.bfloat16).float().numpy())
    # writeObject / readObject
    q2 = sk.ZipMLQuantizer.readObject(q.writeObject())
    assert isinstance(q2, sk.ZipMLQuantizer) and np.array_equal(_bits(q2.getSplits()), _bits(sp))
    assert np.array_equal(q2.getBins().cpu().numpy(), bins) and (q2.getMin(), q2.getMax()) == (h.min, h.max)
    # decode-sum of two Zip payloads
    L = _L()
    q3 = sk.ZipMLQuantizer(256)
    q3.quantize(_dev(y))
    h3, sp3, bins3 = _parse(q3.payload)
    vals3 = Z.ZipResult(Z.OK, h3.bin_num, sp3, h3.min, h3.max, h3.zero_idx).values()
    stride = q.payload.numel()
    assert q3.payload.numel() == stride and stride % 256 == 0
    from sketchml_amd.context import alloc_aligned
    both = alloc_aligned(2 * stride, "cuda")
    both[:stride].copy_(q.payload)
    both[stride:].copy_(q3.payload)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    assert L.lib.skml_dense_decode_sum_f32(_ctx().handle, _ptr(both), 2, stride, _ptr(out), n, 0.5) == 0, L.last_error()
    assert np.array_equal(out.cpu().numpy(), ((0.0 + vals[bins] + vals3[bins3]) * 0.5).astype(np.float32))
    # timesBy
    q.timesBy(-0.25)
    assert np.array_equal(q.getSplits(), sp * -0.25) and (q.getMin(), q.getMax()) == (h.min * -0.25, h.max * -0.25)
    # fp64 input decodes to doubles; bf16 input is widened
    q4 = sk.ZipMLQuantizer(16)
    q4.quantize(_dev(_gauss(4097, "f64")))
    assert q4.decode().dtype == torch.float64
    xb = torch.from_numpy(_gauss(4097, "f32")).to(torch.bfloat16)
    q5, q6 = sk.ZipMLQuantizer(16), sk.ZipMLQuantizer(16)
    q5.quantize(xb.cuda())
    q6.quantize(xb.float().cuda())
    _same_payload(q5.payload, q6.payload)
    with pytest.warns(UserWarning, match="sequential"):
        q6.parallelQuantize(xb.float().cuda())
    _same_payload(q5.payload, q6.payload)


# ---- 7. refusals ----
def _ok_after():
    st, _ = _encode(_gauss(300, "f32"), 16)
    assert st == 0, f"the context is not usable after a refusal: {_L().last_error()}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nan_and_infinity_are_refused(bad, kind):
    L = _L()
    n = 8193
    for pos in (0, n // 2, n - 1):
        x = _gauss(n, kind).copy()
        x[pos] = bad
        st, _ = _encode(x, 256)
        assert st == L.SKML_E_NAN, (pos, st, L.last_error())
        _ok_after()


def test_inputs_the_reference_never_finishes_are_refused():
    import sketchml_amd as sk
    L = _L()
    for x in (np.full(300, 0.25, dtype=np.float32), Z.mostly_zeros()):
        assert Z.quantize(x, 256).status == Z.NO_PROGRESS
        st, _ = _encode(x, 256)
        assert st == L.SKML_E_ARG and "does not terminate" in L.last_error(), (st, L.last_error())
        _ok_after()
    # a stall in a round that runs in global memory (splitNum > 4,096), and through the Python class
    x = np.zeros(20000, dtype=np.float32)
    x[::500] = 1.0
    assert Z.quantize(x, 256).status == Z.NO_PROGRESS
    with pytest.raises(sk.SketchMLException, match="does not terminate"):
        sk.ZipMLQuantizer(256).quantize(_dev(x))
    _ok_after()


def test_argument_checks():
    L = _L()
    x = _gauss(300, "f32")
    for bins in (2, 3, 65537):
        from sketchml_amd.context import alloc_aligned
        xd, pl = _dev(x), alloc_aligned(1 << 20, "cuda")
        assert L.lib.skml_zip_encode_f32(_ctx().handle, _ptr(xd), 300, bins, _ptr(pl), 1 << 20) == L.SKML_E_ARG
        _ok_after()
    xd, pl = _dev(x), alloc_aligned(1 << 20, "cuda")
    assert L.lib.skml_zip_encode_f32(_ctx().handle, _ptr(xd), 1, 256, _ptr(pl), 1 << 20) == L.SKML_E_ARG
    _ok_after()
    st, _ = _encode(x, 256, cap_delta=-1)
    assert st == L.SKML_E_ARG and "capacity" in L.last_error()
    _ok_after()


# ---- 8. determinism ----
def test_five_encodes_give_the_same_bytes():
    x = _gauss((1 << 20) + 1, "f32")
    first = None
    for _ in range(5):
        st, pl = _encode(x, 256)
        assert st == 0
        b = pl.cpu()
        first = b if first is None else first
        assert torch.equal(b, first)


# ---- 9. stream order ----
N_ORDER = 3 * 8192 + 77


@functools.lru_cache(maxsize=None)
def _order_expect(kind):
    x = _gauss(N_ORDER, kind)
    return Z.quantize(x, 256, *_hook(x))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pattern", ["A", "B"])
def test_stream_order(sl, pattern, kind):  # noqa: F811
    """tests/test_gpu_stream_order.py's two patterns: A, the input arrives behind a delay on the
    context's own non-blocking stream (the stale input is another valid data set); B, a busy null
    stream, a fresh context, recycled 0xFF memory, a 0xFF payload."""
    from sketchml_amd.context import alloc_aligned
    L = _L()
    z = _order_expect(kind)
    fresh = _gauss(N_ORDER, kind)
    stale = (_gauss(N_ORDER + 1, kind)[:N_ORDER] * 3 + fresh.dtype.type(1e-3)).astype(fresh.dtype)
    nb = L.lib.skml_dense_payload_bytes(N_ORDER, 256)
    pl = alloc_aligned(nb, "cuda").fill_(0xFF)
    xin = _dev(stale if pattern == "A" else fresh)
    fresh_dev = _dev(fresh)
    name = "skml_zip_encode_f64" if kind == "f64" else "skml_zip_encode_f32"

    def call(h):
        sl.c(name, h, _ptr(xin), N_ORDER, 256, _ptr(pl), nb)

    if pattern == "A":
        got = run_a(sl, [(xin, fresh_dev)], call, lambda: [pl], scribble=[pl], host_sync=True)
    else:
        got, _ = run_b(sl, call, lambda: [pl], host_sync=True)
    h, sp, bins = _parse(got[0])
    assert (h.bin_num, h.zero_idx) == (z.bin_num, z.zero_idx) and np.array_equal(_bits(sp), _bits(z.splits))
    assert np.array_equal(_bits([h.min, h.max]), _bits([z.min, z.max])) and np.array_equal(bins, z.bins(fresh))


def test_stale_workspace_and_release():
    """The context keeps the ZipML workspace between calls: an encode that finds it full of another
    (larger) input's keys, sums and splitIndex gives the payload a fresh context gives, and so does
    the encode after the workspace was released."""
    from sketchml_amd.context import Context
    L = _L()
    other = _gauss(65539, "f64") * 7.0 + 1.0
    for kind in KINDS:
        x = _gauss(3 * 8192 + 77, kind)
        used, fresh = Context(0), Context(0)
        st, _ = _encode(other, 16, used.handle)
        assert st == 0, L.last_error()
        st, a = _encode(x, 256, used.handle)
        assert st == 0, L.last_error()
        st, b = _encode(x, 256, fresh.handle)
        assert st == 0, L.last_error()
        _same_payload(a, b)
        assert L.lib.skml_zip_release_workspace(used.handle) == 0 and L.lib.skml_zip_release_workspace(used.handle) == 0
        st, c = _encode(x, 256, used.handle)
        assert st == 0, L.last_error()
        _same_payload(c, b)


# ---- 10. ZipGradient ----
def test_zip_gradient():
    import sketchml_amd as sk
    dim = 65539
    x = _gauss(dim, "f64")
    z = Z.quantize(x, 256, *_hook(x))
    want = z.values()[z.bins(x)]
    g = sk.ZipGradient(sk.DenseDoubleGradient(dim, _dev(x)), 256)
    assert g.kind() == sk.Kind.Zip and g.countNNZ() == dim and g.indices is None
    assert np.array_equal(g.toDense().values.cpu().numpy(), want)
    auto = g.toAuto()
    assert auto.kind() == sk.Kind.DenseDouble and np.array_equal(auto.values.cpu().numpy(), want)
    with pytest.raises(sk.SketchMLException):
        g.toSparse()
    g.timesBy(2.0)
    assert np.array_equal(g.toDense().values.cpu().numpy(), want * 2.0)
    # sparse: the indices are kept as they are
    keys = np.sort(np.random.default_rng(3).choice(dim, 5000, replace=False)).astype(np.int32)
    vals = _gauss(5000, "f64")
    zs = Z.quantize(vals, 16, *_hook(vals))
    kd = _dev(keys)
    gs = sk.ZipGradient(sk.SparseDoubleGradient(dim, kd, _dev(vals)), 16)
    sp = gs.toSparse()
    assert sp.indices is kd and gs.countNNZ() == 5000
    wants = zs.values()[zs.bins(vals)]
    assert np.array_equal(sp.values.cpu().numpy(), wants)
    auto = gs.toAuto()
    assert auto.kind() == sk.Kind.SparseDouble and np.array_equal(auto.values.cpu().numpy(), wants)
    # ZipGradient.scala:43-47 as written: toDense of a sparse-built gradient wraps the `size` decoded values
    assert np.array_equal(gs.toDense().values.cpu().numpy(), wants)
    with pytest.raises(sk.SketchMLException, match="Cannot create Zip"):
        sk.ZipGradient(g, 16)
