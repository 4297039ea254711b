"""The mini-batch gradient on the device (skml_glm_gradient_*, skml_glm_finish_*, optim.GradientDescent.
miniBatchGradientDescent) against tests/glm_ref.py, bit for bit wherever Java pins the bits:

- pre for every loss; coef and loss_j for the hinge and the square loss;
- coef and loss_j of the log losses to |coef - ref| <= 2^-50 |ref| and |loss - ref| <= 2^-50 (1 + |ref|):
  Math.exp / Math.log, numpy's and the device's are each within 1 ulp, and the add, the divide and
  the log round once each, so either side is within 2^-51 of the exact value;
- grad_out, nnz, toAuto's form and the finished gradient against the reference fed the device's coef;
- objLoss and regLoss to |dev - fsum(terms)| <= (n - 1) 2^-53 sum|term|, which holds for any order.

The data sets are tests/glm_fixtures.py's, whose sums depend on the order of their additions
(tests/test_glm_cpu.py::test_fixture_sums_depend_on_the_order)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import glm_fixtures as FX
import glm_ref as R

pytestmark = pytest.mark.gpu

LAM = 0.0078125


def _L():
    from sketchml_amd import _lib
    return _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _raw(name):
    if name == "bias":
        return FX.bias_data()
    if name == "tiny":
        return FX.tiny_data()
    if name == "exact":  # window (0, 20) hits 20 of 30 columns, (0, 21) hits 21: toAuto's threshold
        rows = 40
        col = np.array([r % 30 for r in range(rows)], dtype=np.int32)
        return (np.arange(rows + 1, dtype=np.int64), col, np.full(rows, 1.5), np.where(np.arange(rows) % 2, 1.0, -1.0)), 30
    return FX.lengths_data(name)


@functools.lru_cache(maxsize=None)
def _dataset(name):
    from sketchml_amd.data import DataSet
    data, dim = _raw(name)
    return DataSet.fromCSR(*data, dim, device="cuda")


@functools.lru_cache(maxsize=None)
def _weights(name, dt):
    dim = _raw(name)[1]
    w = np.zeros(dim) if name == "exact" else FX.weights(dim)
    return w.astype(np.float32 if dt == "f32" else np.float64)


@functools.lru_cache(maxsize=None)
def _weights_dev(name, dt):
    return torch.from_numpy(_weights(name, dt)).cuda()


@functools.lru_cache(maxsize=None)
def _predicted(name, dt, r0, batch, kind):
    data = _raw(name)[0]
    rows, _ = R.window_rows(len(data[3]), r0, batch)
    return (rows,) + R.predict(data, _weights(name, dt), rows, kind)


def _loss(kind, lam=0.0):
    from sketchml_amd import loss as Lo
    return {R.L1_LOG: Lo.L1LogLoss, R.L2_HINGE: Lo.L2HingeLoss, R.L2_LOG: Lo.L2LogLoss, R.L2_SQUARE: Lo.L2SquareLoss}[kind](lam)


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} against {want.shape}"
    bad = np.nonzero(R.bits(got) != R.bits(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, the first at {bad[0]}: {got[bad[0]]!r} against {want[bad[0]]!r}"


def _sum_bound(dev, terms, what):
    terms = np.asarray(terms, dtype=np.float64)
    exact, bound = math.fsum(terms), (len(terms) - 1) * 2.0 ** -53 * math.fsum(np.abs(terms))
    print(f"{what}: device {dev!r}, exactly {exact!r}, off by {abs(dev - exact):.3e} of {bound:.3e} allowed")
    assert abs(dev - exact) <= bound, what


def _check_finish(name, dt, out, g_ref, batch):
    """toAuto's form of the device's unscaled gradient, then timesBy(1 / batch) and each regulariser
    through the finish entries, against the reference on the same form."""
    from sketchml_amd import optim
    from sketchml_amd.gradient import DenseDoubleGradient, SparseDoubleGradient, auto_dense
    from sketchml_amd.sparse import to_sparse
    dim, w, wd = len(g_ref), _weights(name, dt), _weights_dev(name, dt)
    form, keys, vals = R.to_auto(g_ref)
    assert out["nnz"] == R.count_nnz(g_ref)
    assert auto_dense(out["nnz"], dim) == (form == "dense")
    for reg_kind, lam in ((R.L2_LOG, 0.0), (R.L1_LOG, LAM), (R.L2_HINGE, LAM)):
        loss = _loss(reg_kind, lam)
        if form == "dense":
            grad = DenseDoubleGradient(dim, out["grad"].clone())
        else:
            k, v = to_sparse(out["grad"])
            assert np.array_equal(k.cpu().numpy(), keys)
            grad = SparseDoubleGradient(dim, k, v.clone())
        optim.finish_gradient(grad, 1.0 / batch, loss, wd)
        _same(grad.values.cpu().numpy(), R.finish(keys, vals, 1.0 / batch, loss.reg_kind(), lam, w), f"{form} finish, reg {loss.reg_kind()}")
    return form


def _check(name, dt, r0, batch, kind):
    from sketchml_amd import optim
    ds, data = _dataset(name), _raw(name)[0]
    out = optim.batch_gradient(_weights_dev(name, dt), ds, r0, batch, _loss(kind), want_pre=True)
    rows, pre, coef, loss = _predicted(name, dt, r0, batch, kind)
    d_pre, d_coef, d_loss = (out[k].cpu().numpy() for k in ("pre", "coef", "loss"))
    _same(d_pre, pre, "pre")
    if kind in (R.L2_HINGE, R.L2_SQUARE):
        _same(d_coef, coef, "coef")
        _same(d_loss, loss, "loss")
    else:
        ec = np.abs(d_coef - coef) / np.maximum(np.abs(coef), 5e-324)
        el = np.abs(d_loss - loss) / (1.0 + np.abs(loss))
        print(f"log loss against numpy: coef off by {ec.max() * 2.0 ** 53:.3f} x 2^-53 relative, "
              f"loss by {el.max() * 2.0 ** 52:.3f} x 2^-52 (1 + |ref|)")
        assert np.all(np.abs(d_coef - coef) <= 2.0 ** -50 * np.abs(coef)), "coef of a log loss"
        assert np.all(np.abs(d_loss - loss) <= 2.0 ** -50 * (1.0 + np.abs(loss))), "loss of a log loss"
    g_ref = R.plus_by(data, ds.dim, rows, d_coef)  # everything downstream of coef is exact given the device's own
    _same(out["grad"].cpu().numpy(), g_ref, "grad_out")
    _sum_bound(out["objLoss"], d_loss, "objLoss")
    return _check_finish(name, dt, out, g_ref, batch), out


# the bias column's window is the batch: 1, the lane form's limit 32 and 33, a wave's chunk 64 and 65,
# the wave form's step 256 and 257, 600; r0 = 0, mid-set, a wrap, batch == rows with r0 != 0
BIAS_WINDOWS = [(0, 64), (100, 257), (500, 600), (5, 700), (333, 1), (699, 1), (690, 32), (10, 33), (650, 65), (200, 256)]


@pytest.mark.parametrize("r0,batch", BIAS_WINDOWS)
def test_windows_with_a_bias_column(gpu, r0, batch):
    form, _ = _check("bias", "f64", r0, batch, R.L2_LOG)
    assert form == "sparse"  # most columns are empty


@pytest.mark.parametrize("filler", ["short", "mid", "long"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_row_lengths_in_every_lane_form(gpu, filler, dt):
    """Rows of 0, 1, 63, 64, 65 and 200 entries with one, 8 and 64 lanes per row (the data set's mean
    row length picks the form), in a window that wraps."""
    data, _ = FX.lengths_data(filler)
    rows = len(data[3])
    lens = np.diff(data[0])
    assert set(FX.SPECIAL_LENGTHS) <= set(lens.tolist())
    mean = len(data[1]) // rows
    assert (1 if mean <= 4 else 8 if mean <= 32 else 64) == {"short": 1, "mid": 8, "long": 64}[filler]
    _check(filler, dt, rows // 2, rows - 3, R.L2_SQUARE)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("kind", [R.L1_LOG, R.L2_HINGE, R.L2_LOG, R.L2_SQUARE])
def test_losses_and_weight_types(gpu, kind, dt):
    _check("bias", dt, 450, 400, kind)  # wraps
    _check("long", dt, 0, 130, kind)


def test_every_column_hit_is_dense(gpu):
    form, out = _check("tiny", "f64", 40, 30, R.L2_HINGE)
    assert form == "dense"
    form, _ = _check("tiny", "f32", 0, 50, R.L1_LOG)
    assert form == "dense"


def test_to_auto_at_the_threshold(gpu):
    """nnz == dim * 2 / 3 = 20 stays sparse, 21 is dense (hinge loss at w = 0: coef = -y, every value 1.5)."""
    form, out = _check("exact", "f64", 0, 20, R.L2_HINGE)
    assert (form, out["nnz"]) == ("sparse", 20)
    form, out = _check("exact", "f64", 0, 21, R.L2_HINGE)
    assert (form, out["nnz"]) == ("dense", 21)
    form, out = _check("exact", "f64", 30, 30, R.L2_HINGE)  # wraps: columns 0 .. 9 twice, 10 .. 19 once
    assert (form, out["nnz"]) == ("sparse", 20)


def test_finish_entries_alone(gpu):
    """timesBy and the regularisers on -0.0, +-theta, the values next to them, values that underflow to
    -0.0 under timesBy, with a double and a float weight, dense and keys + values."""
    from sketchml_amd.context import get_context
    L, h = _L(), get_context().handle
    theta = 0.3
    up, down = np.nextafter(theta, np.inf), np.nextafter(theta, -np.inf)
    v = np.array([-0.0, 0.0, theta, -theta, up, -up, down, -down, -5e-324, 5e-324, 1.0, -1.0, 2.0 * theta, -2.0 * theta,
                  1e-9, -1e-9, np.inf, -np.inf, 0.25, -0.125, 3.0])
    n = len(v)
    dim = 4 * n
    keys = (np.arange(n) * 4 + 3).astype(np.int32)
    w64 = FX.weights(dim, seed=9) * 2.0 ** 12
    for w in (w64, w64.astype(np.float32)):
        wd = torch.from_numpy(w).cuda()
        for times in (1.0, 0.5, 1.0 / 3.0):
            for reg in (R.REG_NONE, R.REG_L1, R.REG_L2):
                g = torch.from_numpy(v.copy()).cuda()
                st = L.lib.skml_glm_finish_kv_f64(h, _ptr(torch.from_numpy(keys).cuda()), _ptr(g), n, dim, times, reg, theta,
                                                  _ptr(wd), int(w.dtype == np.float32))
                assert st == 0, L.last_error()
                _same(g.cpu().numpy(), R.finish(keys, v, times, reg, theta, w), f"kv, reg {reg}, times {times}")
                g = torch.from_numpy(v.copy()).cuda()
                st = L.lib.skml_glm_finish_dense_f64(h, _ptr(g), n, times, reg, theta, _ptr(wd), int(w.dtype == np.float32))
                assert st == 0, L.last_error()
                _same(g.cpu().numpy(), R.finish(None, v, times, reg, theta, w), f"dense, reg {reg}, times {times}")
    # L1 is the identity but for -0.0, which -5e-324 * 0.5 also gives
    out = R.finish(None, v, 0.5, R.REG_L1, theta, None)
    assert R.bits(out[[0, 8]]).tolist() == [0, 0] and R.bits(R.finish(None, v, 0.5, R.REG_NONE, theta, None)[[0, 8]]).tolist() == [1 << 63] * 2


def test_bad_arguments_leave_the_gradient_untouched(gpu):
    from sketchml_amd.context import get_context
    L, h = _L(), get_context().handle
    ds = _dataset("bias")
    w = _weights_dev("bias", "f64")
    mark = 123.456
    grad = torch.full((ds.dim,), mark, dtype=torch.float64, device="cuda")
    coef = torch.full((700,), mark, dtype=torch.float64, device="cuda")
    nnz, obj = C.c_int64(-7), C.c_double(-7.0)

    def call(data=None, row0=0, batch=10, kind=R.L2_LOG, wp=None, g=None, fn="skml_glm_gradient_f64", ctx=h, coef_p=None, nz=nnz):
        d = data if data is not None else ds.glm_data()
        return getattr(L.lib, fn)(ctx, C.byref(d), row0, batch, kind, wp if wp is not None else _ptr(w), None,
                                  coef_p if coef_p is not None else _ptr(coef), None, g if g is not None else _ptr(grad),
                                  C.byref(nz) if nz is not None else None, C.byref(obj))

    def edited(**kw):
        d = ds.glm_data()
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    off4 = lambda t: C.c_void_p(t.data_ptr() + 4)  # noqa: E731
    cases = {
        "ctx NULL": dict(ctx=None),
        "row_ptr NULL": dict(data=edited(row_ptr=None)),
        "csc_val NULL": dict(data=edited(csc_val=None)),
        "w NULL": dict(wp=C.c_void_p(0)),
        "nnz_out NULL": dict(nz=None),
        "val misaligned": dict(data=edited(val=ds.val.data_ptr() + 4)),
        "col_ptr misaligned": dict(data=edited(col_ptr=ds.col_ptr.data_ptr() + 4)),
        "w misaligned": dict(wp=off4(w)),
        "grad misaligned": dict(g=off4(grad)),
        "coef misaligned": dict(coef_p=off4(coef)),
        "row0 < 0": dict(row0=-1),
        "row0 == rows": dict(row0=700),
        "batch 0": dict(batch=0),
        "batch > rows": dict(batch=701),
        "dim beyond a Java int": dict(data=edited(dim=1 << 31)),
        "rows beyond a Java int": dict(data=edited(rows=1 << 31)),
        "dim 0": dict(data=edited(dim=0)),
        "nnz < 0": dict(data=edited(nnz=-1)),
        "unknown loss": dict(kind=4),
        "negative loss": dict(kind=-1),
        "grad is w": dict(g=_ptr(w)),
        "grad inside val": dict(g=_ptr(ds.val)),
        "grad is col_ptr": dict(g=_ptr(ds.col_ptr)),
        "grad overlaps coef": dict(coef_p=_ptr(grad)),
        "f32 entry, grad is w": dict(fn="skml_glm_gradient_f32", g=_ptr(w)),
    }
    before = {k: getattr(ds, k).clone() for k in ("val", "col_ptr")}
    w_before = w.clone()
    for what, kw in cases.items():
        assert call(**kw) == L.SKML_E_ARG, f"{what}: {L.last_error()}"
        assert L.last_error(), what
    torch.cuda.synchronize()
    assert bool((grad == mark).all()) and bool((coef == mark).all()) and (nnz.value, obj.value) == (-7, -7.0)
    assert torch.equal(w, w_before) and all(torch.equal(getattr(ds, k), t) for k, t in before.items())
    # the finish entries
    v = torch.full((64,), mark, dtype=torch.float64, device="cuda")
    k = torch.arange(64, dtype=torch.int32, device="cuda")
    wv = torch.zeros(64, dtype=torch.float64, device="cuda")
    fd, fk = L.lib.skml_glm_finish_dense_f64, L.lib.skml_glm_finish_kv_f64
    assert fd(h, _ptr(v), 64, 0.5, 3, 0.1, _ptr(wv), 0) == L.SKML_E_ARG  # an unknown regulariser
    assert fd(h, None, 64, 0.5, 0, 0.1, None, 0) == L.SKML_E_ARG
    assert fd(h, off4(v), 32, 0.5, 0, 0.1, None, 0) == L.SKML_E_ARG
    assert fd(h, _ptr(v), 0, 0.5, 0, 0.1, None, 0) == L.SKML_E_ARG
    assert fd(h, _ptr(v), 64, 0.5, R.REG_L2, 0.1, None, 0) == L.SKML_E_ARG  # L2 needs w
    assert fd(h, _ptr(v), 64, 0.5, R.REG_L2, 0.1, _ptr(v), 0) == L.SKML_E_ARG  # the values are w
    assert fk(h, None, _ptr(v), 64, 64, 0.5, 0, 0.1, None, 0) == L.SKML_E_ARG
    assert fk(h, _ptr(k), _ptr(v), 65, 64, 0.5, 0, 0.1, None, 0) == L.SKML_E_ARG
    assert fk(h, _ptr(k), _ptr(v), 64, 64, 0.5, -1, 0.1, None, 0) == L.SKML_E_ARG
    torch.cuda.synchronize()
    assert bool((v == mark).all())
    # and the same arguments made right are accepted
    assert call() == 0 and nnz.value > 0
    assert fk(h, _ptr(k), _ptr(v), 64, 64, 0.5, R.REG_L2, 0.1, _ptr(wv), 0) == 0
    assert bool((v.cpu() == mark * 0.5).all())


@pytest.mark.parametrize("kind,lam", [(R.L1_LOG, LAM), (R.L2_HINGE, LAM), (R.L2_SQUARE, 0.0)])
def test_mini_batch_gradient_descent_continues_the_read_index(gpu, kind, lam):
    """Two consecutive calls (batch 420 of 700: rows 0 .. 419, then 420 .. 699 and 0 .. 139), each against the
    reference fed the device's coef of the same window; regLoss through the sqrt and the product."""
    import sketchml_amd as sk
    from sketchml_amd import optim
    from sketchml_amd.data import DataSet
    data, dim = FX.bias_data()
    ds = DataSet.fromCSR(*data, dim, device="cuda")
    w, wd = _weights("bias", "f32"), _weights_dev("bias", "f32")
    loss = _loss(kind, lam)
    opt = sk.GradientDescent(dim, 0.1, 0.5, 0.6)
    assert opt.batchNum == 2.0
    for step, (r0, after, epoch, batch_no) in enumerate([(0, 420, 0, 1), (420, 140, 1, 0)]):
        grad, batch, obj, reg = opt.miniBatchGradientDescent(wd, ds, loss)
        assert batch == 420 and ds.readIndex == after and (opt.epoch, opt.batch) == (epoch, batch_no)
        ref = optim.batch_gradient(wd, ds, r0, batch, loss)
        assert obj == ref["objLoss"] and torch.equal(opt.lastLoss, ref["loss"])  # the same bits run to run
        rows, _ = R.window_rows(700, r0, batch)
        g_ref = R.plus_by(data, dim, rows, ref["coef"].cpu().numpy())
        form, keys, vals = R.to_auto(g_ref)
        assert form == "sparse" and grad.kind() == sk.Kind.SparseDouble and grad.values.dtype == torch.float64
        assert np.array_equal(grad.indices.cpu().numpy(), keys)
        _same(grad.values.cpu().numpy(), R.finish(keys, vals, 1.0 / batch, loss.reg_kind(), lam, w), f"step {step}")
        terms, exact = R.reg_loss(loss.reg_kind(), lam, w)
        if loss.reg_kind() == R.REG_NONE:
            assert reg == 0.0
            continue
        s, b = math.fsum(terms), (len(terms) - 1) * 2.0 ** -53 * math.fsum(np.abs(terms))
        f = (lambda x: x) if loss.reg_kind() == R.REG_L1 else math.sqrt
        lo, hi = f(s - b) * lam * (1 - 2.0 ** -51), f(s + b) * lam * (1 + 2.0 ** -51)  # two roundings after the sum
        print(f"regLoss {reg!r}, exactly {exact!r}, allowed [{lo!r}, {hi!r}]")
        assert lo <= reg <= hi


def test_one_training_step_twice(gpu):
    """miniBatchGradientDescent -> compress(grad, "Sketch") -> toAuto -> Adam.update, run twice from the
    same state: the same weight, moments and logged scalars bit for bit."""
    import sketchml_amd as sk
    from sketchml_amd.data import DataSet
    data, dim = FX.bias_data()
    results = []
    for _ in range(2):
        ds = DataSet.fromCSR(*data, dim, device="cuda")
        w = torch.from_numpy(FX.weights(dim)).cuda()
        opt = sk.Adam(dim, 0.01, 0.0, 0.8)
        grad, batch, obj, reg = opt.miniBatchGradientDescent(w, ds, sk.L2LogLoss(LAM))
        sketch = sk.compress(grad, "Sketch", seed=3, hashSeed=4)
        assert sketch.kind() == sk.Kind.Sketch
        opt.update(sketch.toAuto(), w)
        torch.cuda.synchronize()
        results.append((batch, obj, reg, w.cpu().numpy(), opt.m.cpu().numpy(), opt.v.cpu().numpy()))
    a, b = results
    assert a[0] == b[0] == 560 and a[1] == b[1] and a[2] == b[2] and a[2] > 0.0
    for x, y, what in zip(a[3:], b[3:], "wmv"):
        _same(x, y, what)
    assert not np.array_equal(a[3], FX.weights(dim)) and np.count_nonzero(a[4]) > 40
