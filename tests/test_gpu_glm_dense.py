"""The dense entries (skml_glm_gradient_dense_*, skml_glm_validate_dense_*, data.DenseDataSet) against
tests/glm_ref.py fed the same rows as a CSR that stores every column, bit for bit wherever Java pins the
bits: everything for the hinge and the square loss; pre, and grad given the device's own coef, for the
log losses (as tests/test_gpu_glm.py).  Values are normal draws times 2^e, e in [-12, 12], so the order
of the additions decides the bits (asserted in _case).  Shapes sit around the kernels' constants, read
from the library: C, U, V and the wave counts from which workgroups hold more than one wave."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import glm_ref as R
from sketchml_amd import _lib as L, loss as Lo

pytestmark = pytest.mark.gpu

TILE_C, SUM_U, ROW_GROUP_AT, COL_GROUP_AT = (L.glm_dense_constant(k) for k in ("C", "U", "ROW_GROUP_AT", "COL_GROUP_AT"))
WC = 64 * L.glm_dense_constant("V")
SHAPES = ([(b + 3, d, 2, b, R.L2_SQUARE) for b in (1, 63, 64, 65, 2 * 64 + 1) for d in (1, TILE_C - 1, TILE_C, TILE_C + 1, 2 * TILE_C + 3)]
          + [(b + 2, d, 1, b, R.L2_HINGE) for b in (1, SUM_U - 1, SUM_U, SUM_U + 1, 2 * SUM_U + 1) for d in (1, WC - 1, WC, WC + 1, 2 * WC + 1)])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _loss(kind):
    return getattr(Lo, {R.L1_LOG: "L1LogLoss", R.L2_HINGE: "L2HingeLoss", R.L2_LOG: "L2LogLoss", R.L2_SQUARE: "L2SquareLoss"}[kind])(0.0)


def _same(got, want, what):
    """Bit for bit; a NaN answers a NaN (the sign and payload of a produced NaN are the machine's)."""
    got, want = np.asarray(got.cpu() if torch.is_tensor(got) else got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} against {want.shape}"
    bad = np.nonzero((R.bits(got) != R.bits(want)) & ~(np.isnan(got) & np.isnan(want)))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, the first at {bad[0]}: {got[bad[0]]!r} against {want[bad[0]]!r}"


@functools.lru_cache(maxsize=None)
def _case(rows, dim, special=False):
    """(x, label, w, the full CSR), built once, never modified; special: stored +-0.0 and column dim // 2 all zero;
    special "inf": also an Inf in x against a zero weight.  The full CSR is left out above 10,000 elements."""
    rng = np.random.default_rng(1000 * rows + dim)
    x = rng.standard_normal((rows, dim)) * np.exp2(rng.integers(-12, 13, (rows, dim)).astype(np.float64))
    w = rng.standard_normal(dim) * np.exp2(rng.integers(-12, 13, dim).astype(np.float64))
    label = np.where(rng.random(rows) < 0.5, 1.0, -1.0)
    label[::7] = rng.standard_normal(len(label[::7]))
    if special:
        x[rng.random((rows, dim)) < 0.2] = 0.0
        x[rng.random((rows, dim)) < 0.1] = -0.0
        x[:, dim // 2] = 0.0
    if special == "inf":
        x[5, 9], w[9] = np.inf, 0.0
    if rows * dim >= 10000:
        return x, label, w, None
    csr = (np.arange(rows + 1, dtype=np.int64) * dim, np.tile(np.arange(dim, dtype=np.int32), rows), x.reshape(-1).copy(), label)
    if rows >= 32 and dim >= 8 and not special:  # the order of the additions decides the bits: most columns' sums differ reversed
        cols = R.column_terms(csr, list(range(rows)), label).values()
        assert 2 * sum(R.sum_forward(t) != R.sum_reverse(t) for t in cols) > dim, (rows, dim)
    return x, label, w, csr


@functools.lru_cache(maxsize=None)
def _data(rows, dim, special=False, dense=True):
    from sketchml_amd.data import DataSet, DenseDataSet
    x, label, _, csr = _case(rows, dim, special)
    return DenseDataSet.fromArray(x, label, dim, device="cuda") if dense else DataSet.fromCSR(*csr, dim, device="cuda")


def _w(rows, dim, dt, special=False):
    return _case(rows, dim, special)[2].astype(np.float32 if dt == "f32" else np.float64)


def _check(rows, dim, r0, batch, kind, dt="f64", special=False):
    from sketchml_amd import optim
    w, csr = _w(rows, dim, dt, special), _case(rows, dim, special)[3]
    out = optim.batch_gradient(torch.from_numpy(w).cuda(), _data(rows, dim, special), r0, batch, _loss(kind), want_pre=True)
    win, _ = R.window_rows(rows, r0, batch)
    pre, coef, loss = R.predict(csr, w, win, kind)
    _same(out["pre"], pre, "pre")
    if kind in (R.L2_HINGE, R.L2_SQUARE):
        _same(out["coef"], coef, "coef")
        _same(out["loss"], loss, "loss")
    g_ref = R.plus_by(csr, dim, win, out["coef"].cpu().numpy())
    _same(out["grad"], g_ref, "grad_out")
    assert out["nnz"] == R.count_nnz(g_ref)
    return g_ref


@pytest.mark.parametrize("rows,dim,r0,batch,kind", SHAPES + [(70, 37, r0, b, R.L2_SQUARE) for r0, b in ((0, 70), (13, 70), (69, 1), (69, 2))])
def test_tiles_and_windows(gpu, rows, dim, r0, batch, kind):
    """Around the row dot's tile, then the column sum's (wrapping); batch == rows, the last row alone, an odd dim."""
    _check(rows, dim, r0, batch, kind, special=rows == 70)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("kind", [R.L1_LOG, R.L2_HINGE, R.L2_LOG, R.L2_SQUARE])
def test_losses_and_weight_types(gpu, kind, dt):
    g_ref = _check(200, 37, 150, 130, kind, dt, special=True)
    assert R.bits(g_ref[18:19])[0] == 0  # the all-zero column: +0.0, and _check saw it counted out


@pytest.mark.parametrize("rows,dim", [(64 * ROW_GROUP_AT + 1, 2), (3, 64 * COL_GROUP_AT + 1)])
def test_workgroups_of_more_than_one_wave(gpu, rows, dim):
    """The smallest shapes past each cut (two waves per group of the row dot, gradient and validation; four of
    the column sum) against a numpy chain across all rows or columns at once."""
    from sketchml_amd import optim, validation
    x, y, w, _ = _case(rows, dim)
    wd, r0, win = torch.from_numpy(w).cuda(), rows - 1, np.r_[rows - 1, 0:rows - 1]  # the window wraps after one row
    out = optim.batch_gradient(wd, _data(rows, dim), r0, rows, _loss(R.L2_SQUARE), want_pre=True)
    chain = lambda terms: functools.reduce(np.add, terms, 0.0)  # noqa: E731  (from +0.0, one rounded add after the other)
    pre = chain([w[c] * x[:, c] for c in range(dim)]) if dim == 2 else np.array([R.dot(w, range(dim), x[r]) for r in range(rows)])
    _same(out["pre"], pre[win], "pre")
    _same(out["coef"], -1.0 * (y - pre)[win], "coef")
    if rows == 3:
        _same(out["grad"], chain([x[r] * c for r, c in zip(win, out["coef"].cpu().numpy())]), "grad_out")
    v = validation.calLossPrecision(wd, _data(rows, dim), _loss(R.L2_SQUARE), "tree")
    z = pre * y
    _same(v.pre, pre, "validation pre")
    _same(v.loss, (0.5 * (pre - y)) * (pre - y), "validation loss")
    assert tuple(v)[1:] == (((z > 0) & (pre > 0)).sum(), ((z > 0) & (pre <= 0)).sum(), ((z < 0) & (pre > 0)).sum(), ((z < 0) & (pre <= 0)).sum(), rows)


def test_to_auto_at_the_threshold(gpu):
    """One 1.5 per row at column r % 30, hinge at w = 0 (coef = -y): 20 live values of 30 stay sparse, 21 are dense."""
    import sketchml_amd as sk
    x = np.zeros((40, 30))
    x[np.arange(40), np.arange(40) % 30] = 1.5
    ds = sk.DenseDataSet.fromArray(x, np.where(np.arange(40) % 2, 1.0, -1.0), 30, device="cuda")
    for batch, form in ((20, sk.Kind.SparseDouble), (21, sk.Kind.DenseDouble)):
        ds.readIndex = 0
        grad, n, _, _ = sk.GradientDescent(30, 0.1, 0.0, batch / 40).miniBatchGradientDescent(torch.zeros(30, dtype=torch.float64, device="cuda"), ds, sk.L2HingeLoss(0.0))
        assert n == batch and grad.kind() == form and int((grad.values != 0).sum()) == batch


def test_an_infinity_against_a_zero_weight_is_nan(gpu):
    with np.errstate(invalid="ignore"):
        g_ref = _check(70, 37, 0, 70, R.L2_SQUARE, special="inf")  # pre[5] is NaN on both sides, and nnz == 0: |NaN| > 1e-8 is false
        pre = R.predict(_case(70, 37, "inf")[3], _case(70, 37, "inf")[2], list(range(70)), R.L2_SQUARE)[0]
    assert np.isnan(pre[5]) and np.isnan(pre).sum() == 1 and np.isnan(g_ref).all()  # 0 * NaN reaches every column


@pytest.mark.parametrize("kind,dt", [(R.L2_LOG, "f32"), (R.L2_HINGE, "f64")])
def test_every_output_equals_the_sparse_entries_on_the_full_csr(gpu, kind, dt):
    from sketchml_amd import optim, validation
    w = torch.from_numpy(_w(200, 37, dt, True)).cuda()
    both = (_data(200, 37, True), _data(200, 37, True, dense=False))
    a, b = (optim.batch_gradient(w, ds, 150, 130, _loss(kind), want_pre=True) for ds in both)
    assert (a["nnz"], R.bits([a["objLoss"]])[0]) == (b["nnz"], R.bits([b["objLoss"]])[0])
    for fn, order in ((validation.calLossAucPrecision, "sequential"), (validation.calLossPrecision, "tree")):
        va, vb = (fn(w, ds, _loss(kind), order) for ds in both)
        assert tuple(va) == tuple(vb) and va.validNum == 200 and sum(va[1:5]) > 100
        assert (va.auc, va.M, va.N, va.sigma, va.nanScores) == (vb.auc, vb.M, vb.N, vb.sigma, vb.nanScores)
        for k, p, q in [(k, a[k], b[k]) for k in ("pre", "coef", "loss", "grad")] + [("v.pre", va.pre, vb.pre), ("v.loss", va.loss, vb.loss)]:
            _same(p, q.cpu().numpy(), k)
    _same(va.pre, R.predict(_case(200, 37, True)[3], _w(200, 37, dt, True), list(range(200)), kind)[0], "pre")


def test_bad_arguments_leave_the_outputs_untouched(gpu):
    from sketchml_amd.context import get_context
    h, ds, mark = get_context().handle, _data(70, 37), 123.456
    w = torch.from_numpy(_w(70, 37, "f64")).cuda()
    grad = torch.full((37,), mark, dtype=torch.float64, device="cuda")
    coef, per = (torch.full((70,), mark, dtype=torch.float64, device="cuda") for _ in range(2))
    nnz, obj, res = C.c_int64(-7), C.c_double(-7.0), L.ValidResult(num=-7)

    def edited(**kw):
        return L.GlmDenseData(**{**{f: getattr(ds.glm_data(), f) for f, _ in L.GlmDenseData._fields_}, **kw})

    def gradient(data=None, row0=0, batch=10, kind=R.L2_LOG, wp=None, g=None, ctx=h, fn="skml_glm_gradient_dense_f64"):
        return getattr(L.lib, fn)(ctx, C.byref(data or ds.glm_data()), row0, batch, kind, wp or _ptr(w), None, _ptr(coef), None,
                                  g or _ptr(grad), C.byref(nnz), C.byref(obj))

    def validate(data=None, kind=R.L2_LOG, flags=0, wp=None, per_p=None, ctx=h):
        return L.lib.skml_glm_validate_dense_f64(ctx, C.byref(data or ds.glm_data()), kind, wp or _ptr(w), flags, None,
                                                 per_p or _ptr(per), C.byref(res))

    off4 = lambda t: C.c_void_p(t.data_ptr() + 4)  # noqa: E731
    shared = [dict(ctx=None), dict(data=edited(x=None)), dict(data=edited(label=None)), dict(data=edited(x=ds.x.data_ptr() + 4)),
              dict(wp=off4(w)), dict(data=edited(dim=0)), dict(data=edited(rows=0)), dict(data=edited(dim=1 << 31)),
              dict(data=edited(rows=(1 << 31) - 1, dim=(1 << 31) - 1)),  # rows * dim * 8 beyond an int64
              dict(kind=4)]
    only_gradient = [dict(row0=-1), dict(row0=70), dict(batch=0), dict(batch=71), dict(g=off4(grad)), dict(g=_ptr(w)),
                     dict(g=_ptr(ds.x)), dict(fn="skml_glm_gradient_dense_f32", g=_ptr(coef))]
    for call, cases in ((gradient, shared + only_gradient), (validate, shared + [dict(flags=4), dict(per_p=_ptr(ds.x)), dict(per_p=off4(per))])):
        for kw in cases:
            assert call(**kw) == L.SKML_E_ARG and L.last_error(), f"{call.__name__}, {kw}: {L.last_error()}"
    torch.cuda.synchronize()
    assert all(bool((t == mark).all()) for t in (grad, coef, per)) and (nnz.value, obj.value, res.num) == (-7, -7.0, -7)
    assert gradient() == 0 and nnz.value > 0 and validate() == 0 and res.num == 70  # made right, they are accepted


def test_mini_batch_gradient_descent_continues_the_read_index(gpu):
    """Two calls of 42 of 70 rows: 0 .. 41, then 42 .. 69 and 0 .. 13."""
    import sketchml_amd as sk
    from sketchml_amd import optim
    ds = sk.DenseDataSet.fromArray(*_case(70, 37)[:2], 37, device="cuda")
    w = torch.from_numpy(_w(70, 37, "f32")).cuda()
    loss, opt = _loss(R.L2_HINGE), sk.GradientDescent(37, 0.1, 0.5, 0.6)
    for r0, after in ((0, 42), (42, 14)):
        grad, batch, obj, _ = opt.miniBatchGradientDescent(w, ds, loss)
        assert batch == 42 and ds.readIndex == after and grad.kind() == sk.Kind.DenseDouble
        ref = optim.batch_gradient(w, _data(70, 37), r0, 42, loss)
        ref_grad = sk.DenseDoubleGradient(37, ref["grad"])
        optim.finish_gradient(ref_grad, 1.0 / 42, loss, w)
        _same(grad.values, ref_grad.values.cpu().numpy(), f"the window at {r0}")
        assert obj == ref["objLoss"]


def test_training_run_equals_the_full_csr_run(gpu):
    """LinearRegModel, two epochs, compressor "None": a DenseDataSet and the DataSet that stores every column."""
    import sketchml_amd as sk
    conf = sk.MLConf(sk.LinearRegModel.name, "", "csv", 1, 37, epochNum=2, batchSpRatio=0.25, learnRate=0.1, l2Reg=0.0, compressor="None")
    runs = []
    for dense in (True, False):
        mdl = sk.LinearRegModel(conf, _data(200, 37, True, dense), _data(70, 37, True, dense))
        mdl.trainData.readIndex = 0
        tl, vl, last = mdl.train()
        runs.append((tuple(last), tl, vl, mdl.weights.cpu().numpy(), mdl.optimizer.m.cpu().numpy(), mdl.optimizer.v.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and len(runs[0][1]) == 3 and np.count_nonzero(runs[0][3]) > 0
    for p, q, what in zip(runs[0][1:], runs[1][1:], ("trainLosses", "validLosses", "weights", "m", "v")):
        _same(p, q, what)
