"""The optimiser step fused into the fixed-point decode-sum (skml_fixed_decode_sum_step_f32 / _f64)
against tests/fixed_point_ref.py and tests/optim_ref.py, bit for bit.

The reference of a payload is decode_values(encode_codes(v, bits, seed, norm=header.norm), bits,
header.norm): the codes recomputed in numpy with the norm the device wrote (the device's sum of
squares is a fixed tree, tests/test_gpu_fixed_point.py), never the library's own decode.  The
gradient is optim_ref.gradient of those doubles (summed in payload order, scaled, never rounded to
float), the update optim_ref.step on optim_ref.selection.  Every comparison is on the bit patterns
of w, m and v, from the recognisable non-zero state of tests/test_gpu_optim.py.  Inputs are N(0,1)
fp32: at 3 bits every quotient |v| / norm * 3 is below 1, so a code is its coin flip sigma and about
half of a payload's values decode to +-0.0 -- the dead elements of LIVE and AUTO.
"""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import optim_ref as R
import test_gpu_optim as T
from test_gpu_optim import _release_shared_cases  # noqa: F401  (this module fills T._state's cache)
from tests import fixed_point_ref as F

pytestmark = pytest.mark.gpu

DT = T.DT
N_EDGES = [1, 3, 4, 5, 1023, 1024, 1025, 4097, 65539]  # partial vector, partial round, one / two rounds, workgroups
N_TWO_TRIPS = 2**23 + 1024 + 5  # 2,048 workgroups x 4 waves x 1,024 elements, a round more and a partial one


def _L():
    from sketchml_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _values(n, p, tag=0, mul=1.0):
    rng = np.random.default_rng(100000 * tag + 1000 * p + n)
    v = (rng.standard_normal(n) * mul).astype(np.float32)
    v.setflags(write=False)
    return v


def _reference(slot, v, bits, seed):
    """The decoded doubles of the payload in `slot`, from the norm its header holds now."""
    import sketchml_amd as sk
    h = sk.fixed_point.info(slot)
    return F.decode_values(F.encode_codes(v.astype(np.float64), bits, seed, norm=h.norm), bits, h.norm)


@functools.lru_cache(maxsize=None)
def _gathered(n, bits, P, tag=0, mul=1.0):
    """P distinct payloads (seeds 5 + p) in slots `stride` apart, larger than the payload, and the
    reference's decoded doubles.  Computed once per shape, shared, never modified."""
    import sketchml_amd as sk
    from sketchml_amd.context import alloc_aligned
    nb = sk.fixed_point.payload_bytes(n, bits)
    stride = nb + 256
    allp = alloc_aligned(stride * P, "cuda").zero_()
    decoded = []
    for p in range(P):
        v = _values(n, p, tag, mul)
        slot = allp[p * stride: p * stride + nb]
        sk.fixed_point.encode(torch.from_numpy(np.array(v)).cuda(), bits, 5 + p, out=slot)
        decoded.append(_reference(slot, v, bits, 5 + p))
    torch.cuda.synchronize()
    return allp, stride, tuple(decoded)


@pytest.fixture(scope="module", autouse=True)
def _release_fixed_cases():
    yield
    _gathered.cache_clear()
    _values.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _entry(dt):
    L = _L()
    return L.lib.skml_fixed_decode_sum_step_f64 if dt == "f64" else L.lib.skml_fixed_decode_sum_step_f32


def _fused(gpu, allp, stride, P, n, scale, p, dt, dev):
    st = _entry(dt)(gpu.get_context().handle, T._ptr(allp), P, stride, n, scale, C.byref(p), *(T._ptr(t) for t in dev))
    assert st == 0, _L().last_error()


def _check(gpu, n, bits, P, kind, dt, scale, select=R.ALL, steps=1, pool=None, case=None):
    """`steps` fused steps on one state against the reference; returns (g, mask, (w, m, v))."""
    allp, stride, decoded = case or _gathered(n, bits, pool or P)
    g = R.gradient(decoded[:P], scale)
    p, rp = T._params(kind, select)
    adam = kind == R.ADAM
    mask = R.selection(g, select)
    dev = T._dev(T._state(n, dt), adam)
    want = T._state(n, dt)
    for _ in range(steps):
        _fused(gpu, allp, stride, P, n, scale, p, dt, dev)
        want = R.step(rp, g, want[0], want[1] if adam else None, want[2] if adam else None, mask)
    got = T._host(dev)
    for name, a, b in zip("wmv", got, want):
        if b is not None:
            T._same(a, b, f"{name} (n={n} bits={bits} P={P} kind={kind} {dt} scale={scale} select={select} steps={steps})")
    return g, mask, got


# ---- sizes, widths, payload counts ---------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 3])
@pytest.mark.parametrize("n", N_EDGES)
def test_n_edges(gpu, n, bits):
    _check(gpu, n, bits, 2, R.ADAM, "f32", 0.5)
    _check(gpu, n, bits, 2, R.SGD, "f64", 0.5)


@pytest.mark.parametrize("n", [4097, 65539])
@pytest.mark.parametrize("bits", [2, 4, 8, 16, 3, 7, 13, 29, 9])
def test_widths(gpu, bits, n):
    """2, 4, 8, 16 take the aligned-piece form, 3, 7, 13, 29 straddle words; 8 is the last width with
    its values in LDS, 9 the first that computes them."""
    _check(gpu, n, bits, 2, R.ADAM, "f32", 0.5)
    if bits in (8, 13):
        _check(gpu, n, bits, 2, R.ADAM, "f64", 0.5)


@pytest.mark.parametrize("bits", [8, 3])
@pytest.mark.parametrize("P", [1, 2, 8, 9, 16])
def test_payload_counts(gpu, P, bits):
    """P = 16 at 8 bits is the largest dynamic LDS table: 16 x 256 doubles."""
    _check(gpu, 4097, bits, P, R.ADAM, "f32", 1.0 / P, pool=16)
    _check(gpu, 4097, bits, P, R.SGD, "f64", 1.0 / P, pool=16)


def test_second_trip_of_the_grid(gpu):
    """The grid is capped at 2,048 workgroups: past 2^23 elements a wave takes a second round."""
    _check(gpu, N_TWO_TRIPS, 4, 2, R.SGD, "f32", 0.5)


# ---- selection -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,kind", [("f32", R.ADAM), ("f64", R.ADAM), ("f32", R.SGD), ("f64", R.SGD)])
def test_live_leaves_the_rest_bit_for_bit(gpu, dt, kind):
    n = 65539
    g, mask, (w, m, v) = _check(gpu, n, 3, 1, kind, dt, 1.0, select=R.LIVE, pool=2)
    assert 0.10 < mask.mean() < 0.90, mask.mean()  # the reference has both dead and live elements
    w0, m0, v0 = T._state(n, dt)
    T._same(w[~mask], w0[~mask], "untouched w")
    if kind == R.ADAM:
        T._same(m[~mask], m0[~mask], "untouched m")
        T._same(v[~mask], v0[~mask], "untouched v")
    assert not np.array_equal(w[mask], w0[mask])


@pytest.mark.parametrize("n", [4097, 65539])
def test_auto_takes_both_sides(gpu, n):
    for P, dense in ((1, False), (2, True)):
        _, _, decoded = _gathered(n, 3, 2)
        nnz = int(R.live(R.gradient(decoded[:P], 1.0)).sum())
        print(f"n={n} P={P}: {nnz} live of {n} ({nnz / n:.3f})")
        assert 0 < nnz < n and R.auto_dense(nnz, n) == dense  # the reference's own count lands on this side
        for dt in DT:
            _, mask, _ = _check(gpu, n, 3, P, R.ADAM, dt, 1.0, select=R.AUTO, pool=2)
            assert mask.all() == dense


# ---- the gradient is the double ------------------------------------------------------------------
def test_the_sum_stays_in_double(gpu):
    n, bits, P, scale = 65539, 8, 8, 0.125
    _, _, decoded = _gathered(n, bits, P)
    g = R.gradient(decoded, scale)
    _, rp = T._params(R.ADAM)
    w0, m0, v0 = T._state(n, "f64")
    exact = R.step(rp, g, w0, m0, v0)
    rounded = R.step(rp, g.astype(np.float32).astype(np.float64), w0, m0, v0)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(exact, rounded)), "the float-rounded gradient gives other bits"
    _check(gpu, n, bits, P, R.ADAM, "f64", scale)  # and the device gives the double one's


def test_three_steps_on_one_state(gpu):
    _check(gpu, 65539, 8, 2, R.ADAM, "f32", 0.5, steps=3)


def test_times_by(gpu):
    """A payload whose norm timesBy scaled: the reference takes the header's norm after the call."""
    n, bits = 4097, 8
    allp, stride, decoded = _gathered(n, bits, 2)
    mine = allp.clone()
    nb = gpu.fixed_point.payload_bytes(n, bits)
    slot = mine[stride: stride + nb]
    norm = gpu.fixed_point.info(slot).norm
    codes = F.encode_codes(_values(n, 1).astype(np.float64), bits, 6, norm=norm)  # the codes are the encode's
    gpu.fixed_point.times_by(slot, 1.0 / 3.0)
    after = gpu.fixed_point.info(slot).norm
    assert after == norm * (1.0 / 3.0)
    scaled = F.decode_values(codes, bits, after)
    assert not np.array_equal(scaled, decoded[1])
    for dt in DT:
        _check(gpu, n, bits, 2, R.ADAM, dt, 0.5, case=(mine, stride, (decoded[0], scaled)))


# ---- refusals ------------------------------------------------------------------------------------
def test_refusals(gpu):
    from sketchml_amd.context import alloc_aligned
    L = _L()
    n, bits = 4097, 8
    good, stride, _ = _gathered(n, bits, 2)
    nb = gpu.fixed_point.payload_bytes(n, bits)
    h = gpu.get_context().handle
    p, _ = T._params(R.ADAM)
    sgd, _ = T._params(R.SGD)
    w, m, v = T._dev(T._state(n, "f32"), True)
    before = T._host((w, m, v))
    f32 = L.lib.skml_fixed_decode_sum_step_f32
    x = torch.from_numpy(np.array(_values(n, 1))).cuda()

    def args(pl=good, n_=n, par=p, w_=None, m_=None, v_=None, P=2):
        return (h, T._ptr(pl), P, stride, n_, 0.5, C.byref(par), w_ if w_ is not None else T._ptr(w),
                m_ if m_ is not None else T._ptr(m), v_ if v_ is not None else T._ptr(v))

    assert f32(*args()) == 0, L.last_error()  # the call that the refusals below vary
    w, m, v = T._dev(T._state(n, "f32"), True)

    def second(values, width):
        pl = good.clone()
        gpu.fixed_point.encode(values, width, 6, out=pl[stride: stride + gpu.fixed_point.payload_bytes(len(values), width)])
        return pl

    assert f32(*args(pl=second(x, 3))) == L.SKML_E_ARG and "bits" in L.last_error()           # mixed widths
    assert f32(*args(pl=second(x[:4096], bits))) == L.SKML_E_ARG and "values" in L.last_error()  # mixed n
    bad = np.array(_values(n, 1))
    bad[7] = np.nan
    assert f32(*args(pl=second(torch.from_numpy(bad).cuda(), bits))) == L.SKML_E_NAN             # a refused input
    assert f32(*args(P=0)) == L.SKML_E_ARG
    assert f32(*args(P=17)) == L.SKML_E_ARG
    assert f32(*args(n_=0)) == L.SKML_E_ARG
    assert f32(*args(w_=C.c_void_p(w.data_ptr() + 4))) == L.SKML_E_ARG and "aligned" in L.last_error()
    assert f32(*args(par=sgd)) == L.SKML_E_ARG and "SGD" in L.last_error()                       # m given for SGD
    assert f32(h, T._ptr(good), 2, stride, n, 0.5, C.byref(p), T._ptr(w), None, T._ptr(v)) == L.SKML_E_ARG  # m missing
    assert "Adam" in L.last_error()
    assert f32(*args(m_=T._ptr(w))) == L.SKML_E_ARG and "overlap" in L.last_error()              # w aliasing m
    # w inside the payloads: in the first payload's words, and in the last payload's last bytes
    inside = alloc_aligned(2 * stride + 4 * n, "cuda").zero_()
    inside[:2 * stride].copy_(good)
    for at in (256 + 1024, stride + nb - 16):
        assert f32(*args(pl=inside, w_=C.c_void_p(inside.data_ptr() + at))) == L.SKML_E_ARG and "overlap" in L.last_error()
    assert torch.equal(inside[:2 * stride], good)
    inf, _ = T._params(R.ADAM)
    inf.lr = float("inf")
    assert f32(*args(par=inf)) == L.SKML_E_ARG and "finite" in L.last_error()
    torch.cuda.synchronize()
    for a, b in zip(T._host((w, m, v)), before):  # a refused call changes no state byte
        assert a.tobytes() == b.tobytes()


# ---- Python --------------------------------------------------------------------------------------
def test_decode_sum_update_fixed_point_over_an_epoch_boundary(gpu):
    """Three batches, two per epoch: the third update advances beta_t."""
    from sketchml_amd import distributed as D
    from sketchml_amd import optim
    n, bits, P = 65539, 8, 2
    allp, stride, decoded = _gathered(n, bits, P)
    g = R.gradient(decoded, 1.0 / P)
    h = gpu.get_context().handle
    for dt in DT:
        opt, ref = optim.Adam(n, 0.05, 0.1, 0.5), R.Adam(n, 0.05, 0.1, 0.5)
        w0 = T._state(n, dt)[0]
        w = torch.from_numpy(w0.copy()).cuda()
        want = (w0, np.zeros(n, dtype=w0.dtype), np.zeros(n, dtype=w0.dtype))
        for b in range(3):
            D.decode_sum_update_fixed_point(h, allp, P, stride, n, 1.0 / P, opt, w)
            ref.begin_update()
            want = R.step(ref.params(), g, *want)
            opt.nextBatch()
            ref.next_batch()
            T._same(w.cpu().numpy(), want[0], f"w after batch {b} ({dt})")
        assert (opt.epoch, opt.batch) == (1, 1) and opt.beta1_t == 0.9 * 0.9 and opt.beta2_t == 0.999 * 0.999
        T._same(opt.m.cpu().numpy(), want[1], "m")
        T._same(opt.v.cpu().numpy(), want[2], "v")
    other = optim.GradientDescent(n + 1, 0.05, 0.1, 0.5)
    with pytest.raises(gpu.SketchMLException):
        D.decode_sum_update_fixed_point(h, allp, P, stride, n, 1.0 / P, other, torch.zeros(n + 1, device="cuda"))
