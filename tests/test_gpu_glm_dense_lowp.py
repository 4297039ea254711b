"""The dense entries over an x stored as fp32, bf16 or fp16 (skml_glm_gradient_dense_lowp_*,
skml_glm_validate_dense_lowp_*, data.DenseDataSet(xDtype=...)) against tests/glm_ref.py on the widened array, fed
as the CSR that stores every column, bit for bit as tests/test_gpu_glm_dense.py compares its float64 twin.
Values are normal draws times 2^e rounded to the storage type first (e in [-12, 12], [-8, 8] for fp16, so
nothing rounds to Inf).  Shapes sit around the kernels' constants, read from the library per type.  The data
sets are [:, :dim] views of tensors this file fills with NaN, so every pad element is a NaN."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import glm_ref as R
from sketchml_amd import _lib as L
from test_gpu_glm_dense import _loss, _same
from test_gpu_stream_order import _drain, _ptr, run_a, sl  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu

TYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def K(t, name):
    return L.glm_dense_lowp_constant(L.X_KINDS[TYPES[t]], name)


def _shapes(t):
    c, u, wc = K(t, "C"), K(t, "U"), 64 * K(t, "V")
    return ([(t, b + 3, d, b + 2, b, R.L2_SQUARE) for b in (1, 63, 64, 65, 129) for d in (1, c - 1, c, c + 1, 2 * c + 3)]
            + [(t, b + 2, d, 1, b, R.L2_HINGE) for b in (1, u - 1, u, u + 1, 2 * u + 1) for d in (1, wc - 1, wc, wc + 1, 2 * wc + 1)])


@functools.lru_cache(maxsize=None)
def _case(t, rows, dim, special=False):
    """(the stored x, x widened to float64, label, w, the full CSR of the widened x), built once, never modified.
    special: stored +-0.0, column dim // 2 all zero, the largest finite and the smallest subnormal value of the type
    in rows 2 and 3, and an Inf in row 100 against a zero weight.  The CSR is left out above 40,000 elements."""
    rng, e = np.random.default_rng(1000 * rows + dim), 8 if t == "f16" else 12
    x = rng.standard_normal((rows, dim)) * np.exp2(rng.integers(-e, e + 1, (rows, dim)).astype(np.float64))
    w = rng.standard_normal(dim) * np.exp2(rng.integers(-12, 13, dim).astype(np.float64))
    label = np.where(rng.random(rows) < 0.5, 1.0, -1.0)
    label[::7] = rng.standard_normal(len(label[::7]))
    if special:
        x[rng.random((rows, dim)) < 0.2] = 0.0
        x[rng.random((rows, dim)) < 0.1] = -0.0
        x[:, dim // 2] = 0.0
        x[100, 9], w[9] = np.inf, 0.0
    xs = torch.from_numpy(x).to(TYPES[t])
    if special:
        xs[2, 3] = torch.finfo(TYPES[t]).max
        xs.view(torch.int32 if t == "f32" else torch.int16)[3, 4] = 1  # the smallest subnormal
    xw = xs.double().numpy()
    assert np.isfinite(xw).sum() == xw.size - bool(special) and (not special or 0 < xw[3, 4] < 1e-7)
    csr = (np.arange(rows + 1, dtype=np.int64) * dim, np.tile(np.arange(dim, dtype=np.int32), rows), xw.reshape(-1).copy(), label)
    return xs, xw, label, w, csr if rows * dim < 40000 else None


@functools.lru_cache(maxsize=None)
def _data(t, rows, dim, special=False):
    from sketchml_amd.data import DenseDataSet
    xs, _, label, _, _ = _case(t, rows, dim, special)
    per16 = 16 // xs.element_size()
    buf = torch.full((rows, -(-dim // per16) * per16), float("nan"), dtype=xs.dtype, device="cuda")
    buf[:, :dim] = xs.cuda()
    ds = DenseDataSet.fromArray(buf[:, :dim], label, dim, device="cuda", xDtype=xs.dtype)
    assert ds.glm_data().x == buf.data_ptr() and ds.pitch == buf.shape[1]  # taken as it is, NaN pad included
    return ds


def _check(t, rows, dim, r0, batch, kind, dt="f64", special=False):
    from sketchml_amd import optim
    _, _, _, w, csr = _case(t, rows, dim, special)
    w = w.astype(np.float32 if dt == "f32" else np.float64)
    out = optim.batch_gradient(torch.from_numpy(w).cuda(), _data(t, rows, dim, special), r0, batch, _loss(kind), want_pre=True)
    win, _ = R.window_rows(rows, r0, batch)
    pre, coef, loss = R.predict(csr, w, win, kind)
    _same(out["pre"], pre, "pre")
    if kind in (R.L2_HINGE, R.L2_SQUARE):
        _same(out["coef"], coef, "coef")
        _same(out["loss"], loss, "loss")
    g_ref = R.plus_by(csr, dim, win, out["coef"].cpu().numpy())  # for the log losses: given the device's own coef
    _same(out["grad"], g_ref, "grad_out")
    assert out["nnz"] == R.count_nnz(g_ref)
    return w, g_ref


@pytest.mark.parametrize("t,rows,dim,r0,batch,kind", [s for t in TYPES for s in _shapes(t)])
def test_tiles_and_windows(gpu, t, rows, dim, r0, batch, kind):
    """Around the row dot's tile (windows that start at the last row and wrap), then the column sum's rows in flight and wave."""
    _check(t, rows, dim, r0, batch, kind)


@pytest.mark.parametrize("t", list(TYPES))
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("kind", [R.L1_LOG, R.L2_HINGE, R.L2_LOG, R.L2_SQUARE])
def test_losses_weight_types_and_special_values(gpu, kind, dt, t):
    from sketchml_amd import validation
    w, g_ref = _check(t, 200, 37, 150, 130, kind, dt, special=True)  # rows 150 .. 199 and 0 .. 79: all but the Inf
    assert R.bits(g_ref[18:19])[0] == 0 and np.isfinite(g_ref).all()  # the all-zero column: +0.0, and _check saw it counted out
    v = validation.calLossPrecision(torch.from_numpy(w).cuda(), _data(t, 200, 37, True), _loss(kind))
    with np.errstate(invalid="ignore"):
        pre = R.predict(_case(t, 200, 37, True)[4], w, list(range(200)), kind)[0]
    _same(v.pre, pre, "validation pre")
    assert np.isnan(pre[100]) and np.isnan(pre).sum() == 1 and v.nanScores == 1  # Inf * 0


@pytest.mark.parametrize("t,kind,dt", [("f32", R.L2_LOG, "f32"), ("bf16", R.L2_HINGE, "f64"), ("f16", R.L2_SQUARE, "f32")])
def test_every_output_equals_the_float64_entries_on_the_widened_array(gpu, t, kind, dt):
    """Here through DenseDataSet's own copy (a zero pad) from the widened float64 array, which rounds back exactly."""
    from sketchml_amd import optim, validation
    from sketchml_amd.data import DenseDataSet
    _, xw, label, w, _ = _case(t, 200, 37, True)
    w = torch.from_numpy(w.astype(np.float32 if dt == "f32" else np.float64)).cuda()
    both = [DenseDataSet.fromArray(xw, label, 37, device="cuda", xDtype=d) for d in (TYPES[t], None)]
    a, b = (optim.batch_gradient(w, ds, 150, 130, _loss(kind), want_pre=True) for ds in both)
    assert both[0].entry == "dense_lowp_" and both[0].x.dtype == TYPES[t] and both[1].x.dtype == torch.float64
    assert (a["nnz"], R.bits([a["objLoss"]])[0]) == (b["nnz"], R.bits([b["objLoss"]])[0])
    va, vb = (validation.calLossAucPrecision(w, ds, _loss(kind)) for ds in both)
    _same(np.array([va[0]]), [vb[0]], "validLoss")  # a NaN: the Inf's row is in the sum
    assert tuple(va)[1:] == tuple(vb)[1:] and va.validNum == 200
    assert (va.M, va.N, va.sigma, va.nanScores) == (vb.M, vb.N, vb.sigma, vb.nanScores) and va.nanScores == 1
    for k, p, q in [(k, a[k], b[k]) for k in ("pre", "coef", "loss", "grad")] + [("v.pre", va.pre, vb.pre), ("v.loss", va.loss, vb.loss)]:
        _same(p, q.cpu().numpy(), k)


@pytest.mark.parametrize("t,many_rows", [(t, m) for t in TYPES for m in (True, False)])
def test_workgroups_of_more_than_one_wave(gpu, t, many_rows):
    """The smallest shapes past each cut (two waves per group of the row dot, gradient and validation; four of the
    column sum) against a numpy chain across all rows or columns at once."""
    from sketchml_amd import optim, validation
    rows, dim = (64 * K(t, "ROW_GROUP_AT") + 1, 2) if many_rows else (3, 64 * K(t, "V") * K(t, "COL_GROUP_AT") + 1)
    _, x, y, w, _ = _case(t, rows, dim)
    wd, win = torch.from_numpy(w).cuda(), np.r_[rows - 1, 0:rows - 1]  # the window wraps after one row
    out = optim.batch_gradient(wd, _data(t, rows, dim), rows - 1, rows, _loss(R.L2_SQUARE), want_pre=True)
    chain = lambda terms: functools.reduce(np.add, terms, 0.0)  # noqa: E731  (from +0.0, one rounded add after the other)
    pre = chain([w[c] * x[:, c] for c in range(dim)]) if many_rows else np.array([R.dot(w, range(dim), x[r]) for r in range(rows)])
    _same(out["pre"], pre[win], "pre")
    _same(out["coef"], -1.0 * (y - pre)[win], "coef")
    _same(out["grad"], chain([x[r] * c for r, c in zip(win, out["coef"].cpu().numpy())]), "grad_out")
    v = validation.calLossPrecision(wd, _data(t, rows, dim), _loss(R.L2_SQUARE), "tree")
    _same(v.pre, pre, "validation pre")
    _same(v.loss, (0.5 * (pre - y)) * (pre - y), "validation loss")
    assert v.validNum == rows and sum(tuple(v)[1:5]) == np.count_nonzero(pre * y)


def test_bad_arguments_leave_the_outputs_untouched(gpu):
    from sketchml_amd.context import get_context
    h, ds, mark = get_context().handle, _data("f32", 70, 37), 123.456
    w = torch.from_numpy(_case("f32", 70, 37)[3]).cuda()
    grad = torch.full((37,), mark, dtype=torch.float64, device="cuda")
    coef, per = (torch.full((70,), mark, dtype=torch.float64, device="cuda") for _ in range(2))
    nnz, obj, res = C.c_int64(-7), C.c_double(-7.0), L.ValidResult(num=-7)

    def edited(**kw):
        return L.GlmDenseLowpData(**{**{f: getattr(ds.glm_data(), f) for f, _ in L.GlmDenseLowpData._fields_}, **kw})

    def gradient(data=None, row0=0, batch=10, kind=R.L2_LOG, wp=None, g=None, ctx=h, fn="skml_glm_gradient_dense_lowp_f64"):
        return getattr(L.lib, fn)(ctx, C.byref(data or ds.glm_data()), row0, batch, kind, wp or _ptr(w), None, _ptr(coef), None,
                                  g or _ptr(grad), C.byref(nnz), C.byref(obj))

    def validate(data=None, kind=R.L2_LOG, flags=0, wp=None, per_p=None, ctx=h):
        return L.lib.skml_glm_validate_dense_lowp_f64(ctx, C.byref(data or ds.glm_data()), kind, wp or _ptr(w), flags, None,
                                                      per_p or _ptr(per), C.byref(res))

    off4 = lambda t: C.c_void_p(t.data_ptr() + 4)  # noqa: E731
    assert ds.pitch == 40
    shared = [dict(ctx=None), dict(data=edited(x=None)), dict(data=edited(label=None)), dict(wp=off4(w)), dict(data=edited(dim=0)),
              dict(data=edited(rows=0)), dict(data=edited(dim=1 << 31, pitch=1 << 31)), dict(kind=4),
              dict(data=edited(x_kind=3)), dict(data=edited(x_kind=-1)), dict(data=edited(pitch=36)),  # unknown kind, pitch < dim
              dict(data=edited(pitch=38)), dict(data=edited(x_kind=L.SKML_X_BF16, pitch=44)),         # rows off a 16-byte boundary
              dict(data=edited(x=ds.x.data_ptr() + 4)), dict(data=edited(x=ds.x.data_ptr() + 8)),
              dict(data=edited(rows=(1 << 31) - 1, dim=(1 << 31) - 1, pitch=1 << 31))]                # rows * pitch * 4 beyond an int64
    only_gradient = [dict(row0=-1), dict(row0=70), dict(batch=0), dict(batch=71), dict(g=off4(grad)), dict(g=_ptr(w)),
                     dict(g=_ptr(ds.x)), dict(fn="skml_glm_gradient_dense_lowp_f32", g=_ptr(coef))]
    for call, cases in ((gradient, shared + only_gradient), (validate, shared + [dict(flags=4), dict(per_p=_ptr(ds.x)), dict(per_p=off4(per))])):
        for kw in cases:
            assert call(**kw) == L.SKML_E_ARG and L.last_error(), f"{call.__name__}, {kw}: {L.last_error()}"
    torch.cuda.synchronize()
    assert all(bool((t == mark).all()) for t in (grad, coef, per)) and (nnz.value, obj.value, res.num) == (-7, -7.0, -7)
    assert gradient() == 0 and nnz.value > 0 and validate() == 0 and res.num == 70  # made right, they are accepted


@pytest.mark.parametrize("entry", ["gradient", "validate"])
def test_stream_ordering(gpu, sl, entry):
    """Pattern A of tests/test_gpu_stream_order.py, as tests/test_gpu_glm_dense_stream.py applies it to the float64
    entries: stale weight and labels, the fresh ones copied in behind a sleep on the context's non-blocking stream."""
    from sketchml_amd.data import DenseDataSet
    rows, dim = 200, 37
    xs, _, y_fresh, w_fresh, csr = _case("bf16", rows, dim, True)
    ds = DenseDataSet.fromArray(xs, -3.0 * y_fresh, dim, device="cuda", xDtype=torch.bfloat16)  # the stale labels
    d = ds.glm_data()
    w = torch.from_numpy(_case("bf16", 70, dim)[3].copy()).cuda()                               # the stale weight
    r0, batch = (150, 130) if entry == "gradient" else (0, rows)
    pre, coef, loss = (torch.zeros(batch, dtype=torch.float64, device="cuda") for _ in range(3))
    grad = torch.zeros(dim, dtype=torch.float64, device="cuda")
    nnz, obj, res = C.c_int64(), C.c_double(), L.ValidResult()
    outs = [pre, coef, loss, grad] if entry == "gradient" else [pre, loss]

    def call(h):
        if entry == "gradient":
            sl.c("skml_glm_gradient_dense_lowp_f64", h, C.byref(d), r0, batch, R.L2_SQUARE, _ptr(w), _ptr(pre), _ptr(coef), _ptr(loss),
                 _ptr(grad), C.byref(nnz), C.byref(obj))
        else:
            sl.c("skml_glm_validate_dense_lowp_f64", h, C.byref(d), R.L2_SQUARE, _ptr(w), 0, _ptr(pre), _ptr(loss), C.byref(res))

    got = run_a(sl, [(w, torch.from_numpy(w_fresh).cuda()), (ds.label, torch.from_numpy(y_fresh).cuda())], call, lambda: outs,
                scribble=outs, host_sync=True)
    win, _ = R.window_rows(rows, r0, batch)
    with np.errstate(invalid="ignore"):
        r_pre, r_coef, r_loss = R.predict(csr, w_fresh, win, R.L2_SQUARE)
    want = (r_pre, r_coef, r_loss, R.plus_by(csr, dim, win, r_coef)) if entry == "gradient" else (r_pre, r_loss)
    for a, b in zip(got, want):
        _same(a, b, entry)
    assert nnz.value == R.count_nnz(want[-1]) if entry == "gradient" else (res.num == rows and res.nan_scores == 1)
