"""The sparse mini-batch gradient in the segmented summation order (optim.batch_gradient(order="segmented")).
Feature k has a prescribed number of entries inside the window, placed around the order's constants; the window
starts at the last row, so it wraps after one instance.  Every third feature also stores the 40 rows outside the
window: a long column whatever its window count.  Integer data (magnitude <= 8) sum exactly in any order: bit for bit
against int64 numpy.  Rounded data: m rounded products and m - 1 rounded adds in any order lie within
gamma_m = m u / (1 - m u), u = 2^-53, of the exact integer-arithmetic sum (test_gpu_glm_dense_blocked._ints)."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import glm_ref as R
from sketchml_amd import _lib as L
from test_gpu_glm_dense import _loss, _same
from test_gpu_glm_dense_blocked import K, _ints

pytestmark = pytest.mark.gpu
M_SEQ, SPLIT_AT, SLICE, TILE = (L.glm_segmented_constant(k) for k in ("M_SEQ", "SPLIT_AT", "SLICE", "TILE"))
COUNTS = [0, 1, M_SEQ - 1, M_SEQ, M_SEQ + 1, 63, 64, 65, 129, SPLIT_AT - 1, SPLIT_AT, SPLIT_AT + 1, SLICE + 1, 3 * SLICE + 5, 2, 5]
BATCH, OUTSIDE = max(COUNTS) + 1, 40
ROWS = BATCH + OUTSIDE
WIN = np.r_[ROWS - 1, 0:BATCH - 1]


def _mask(dim, shift):
    """(ROWS x dim stored-entry mask, the features' window counts): feature k holds window positions [0, count)."""
    m = np.array([COUNTS[(k + shift) % len(COUNTS)] for k in range(dim)])
    mask = np.zeros((ROWS, dim), dtype=bool)
    mask[WIN] = np.arange(BATCH)[:, None] < m[None, :]
    mask[BATCH - 1:ROWS - 1, (np.arange(dim) + shift) % 3 == 0] = True
    return mask, m


def _run(x, mask, label, w, kind, order):
    from sketchml_amd import optim
    from sketchml_amd.data import DataSet
    r, c = np.nonzero(mask)
    row_ptr = np.r_[0, np.cumsum(mask.sum(1))].astype(np.int64)
    ds = DataSet.fromCSR(row_ptr, c.astype(np.int32), x[r, c].astype(np.float64), label.astype(np.float64), x.shape[1], device="cuda")
    out = optim.batch_gradient(torch.from_numpy(w).cuda(), ds, ROWS - 1, BATCH, _loss(kind), want_pre=True, order=order)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


@pytest.mark.parametrize("dim,shift", [(1, 4), (1, 10), (1, 13), (TILE - 1, 0), (TILE, 1), (TILE + 1, 2)])
def test_integer_data_equal_the_int64_result_bit_for_bit(gpu, dim, shift):
    rng = np.random.default_rng(dim * 100 + shift)
    mask, _ = _mask(dim, shift)
    x = rng.integers(1, 9, mask.shape) * rng.choice([-1, 1], mask.shape) * mask
    w = rng.integers(-8, 9, dim)
    for kind, label in ((R.L2_HINGE, rng.choice([-1, 1], ROWS)), (R.L2_SQUARE, rng.integers(-8, 9, ROWS))):
        out, seq = (_run(x, mask, label, w.astype(np.float64), kind, order) for order in ("segmented", "sequential"))
        coef = np.array([-1.0 * R.grad_of(kind, p, y) for p, y in zip(x[WIN] @ w, label[WIN])])
        g = x[WIN].T @ coef.astype(np.int64)
        _same(out["grad"], g, "grad")
        assert out["nnz"] == np.count_nonzero(g)
        for name in ("pre", "coef", "loss"):
            _same(out[name], seq[name], name)
        _same(out["coef"], coef, "coef")
        assert out["objLoss"] == seq["objLoss"]


@functools.lru_cache(maxsize=None)
def _rounded():
    rng, dim = np.random.default_rng(7), 2 * len(COUNTS) + 1
    mask, m = _mask(dim, 0)
    x = rng.standard_normal(mask.shape) * np.exp2(rng.integers(-12, 13, mask.shape).astype(np.float64)) * mask
    w = rng.standard_normal(dim) * np.exp2(rng.integers(-4, 5, dim).astype(np.float64))
    return x, mask, m, np.where(rng.random(ROWS) < 0.5, 1.0, -1.0), w, _ints(x[WIN])


@pytest.mark.parametrize("wdt,kind", [(np.float64, R.L2_LOG), (np.float32, R.L2_HINGE), (np.float64, R.L2_SQUARE)])
def test_rounded_data_within_the_bound_of_any_order(gpu, wdt, kind):
    x, mask, m, label, w, xi = _rounded()
    out, seq, again = (_run(x, mask, label, w.astype(wdt), kind, order) for order in ("segmented", "sequential", "segmented"))
    ci = _ints(out["coef"])  # given the device's own coef
    exact, mag = xi.T @ ci, np.abs(xi).T @ np.abs(ci)
    for k in range(x.shape[1]):
        n = max(int(m[k]), 1)
        gamma = Fraction(n, 2 ** 53) / (1 - Fraction(n, 2 ** 53))
        err = abs(Fraction(float(out["grad"][k])) * (1 << 2 * K) - exact[k])
        assert err <= gamma * mag[k], f"feature {k} of {m[k]} entries: {float(err / (gamma * mag[k])):.3g} of its bound"
    _same(out["grad"][m <= M_SEQ], seq["grad"][m <= M_SEQ], "grad of the features of at most M_SEQ entries")
    for name in ("pre", "coef", "loss", "grad"):
        assert np.array_equal(R.bits(out[name]), R.bits(again[name])), name
        if name != "grad":
            _same(out[name], seq[name], name)
    assert out["nnz"] == R.count_nnz(out["grad"]) == again["nnz"] and out["objLoss"] == again["objLoss"] == seq["objLoss"]


def test_inf_times_zero_makes_its_column_nan(gpu):
    """The hinge loss answers a NaN score with coef = -0.0: Inf * -0.0 is NaN in its own column, -0.0 in the others."""
    x, mask, m, label, w, _ = _rounded()
    x, w, hit = x.copy(), w.copy(), [int(np.nonzero(m == c)[0][0]) for c in (5, 3 * SLICE + 5)]
    x[1, hit], w[hit] = np.inf, 0.0
    out = _run(x, mask, label, w, R.L2_HINGE, "segmented")
    assert np.isnan(out["pre"][2]) and np.isnan(out["pre"]).sum() == 1 and sorted(np.nonzero(np.isnan(out["grad"]))[0]) == sorted(hit)


def test_through_the_optimiser_the_model_and_the_refusals(gpu):
    import sketchml_amd as sk
    from sketchml_amd.context import get_context
    from sketchml_amd.data import DenseDataSet
    from sketchml_amd.optim import GradientDescent
    rng, dim = np.random.default_rng(3), 50
    mk = lambda n: sk.DataSet.fromRows([(float(rng.choice([-1, 1])), [0] + sorted(rng.choice(np.arange(1, dim), 4, replace=False)),
                                         rng.standard_normal(5)) for _ in range(n)], dim, device="cuda")
    ds, w0 = mk(200), torch.zeros(dim, dtype=torch.float64, device="cuda")
    grad, batch, obj, _ = GradientDescent(dim, 0.1, 0.9, 0.5).miniBatchGradientDescent(w0, ds, _loss(R.L2_LOG), order="segmented")
    assert batch == 100 and np.isfinite(obj) and bool(torch.isfinite(grad.values).all()) and bool(grad.values.any())
    conf = sk.MLConf(sk.LRModel.name, "", "csv", 1, dim, epochNum=1, batchSpRatio=0.25, learnRate=0.1, l2Reg=0.0, compressor="None")
    mdl = sk.LRModel(conf, mk(200), mk(40), gradientOrder="segmented")
    tl, vl, _ = mdl.train()
    assert np.isfinite(tl + vl).all() and bool(torch.isfinite(mdl.weights).all()) and bool(mdl.weights.any())
    dense = DenseDataSet.fromArray(rng.standard_normal((4, dim)), np.ones(4), dim, device="cuda")
    with pytest.raises(sk.SketchMLException, match="blocked"):
        GradientDescent(dim, 0.1, 0.9, 0.5).miniBatchGradientDescent(w0, dense, _loss(R.L2_LOG), order="segmented")

    d, mark = ds.glm_data(), 123.456
    g, coef = (torch.full((n,), mark, dtype=torch.float64, device="cuda") for n in (dim, 200))
    nnz, objl = C.c_int64(-7), C.c_double(-7.0)

    def call(fn, batch=10, gp=None, **edit):
        data = type(d)(**{**{f: getattr(d, f) for f, _ in d._fields_}, **edit})
        return getattr(L.lib, fn)(get_context().handle, C.byref(data), 0, batch, R.L2_SQUARE, C.c_void_p(w0.data_ptr()), None,
                                  C.c_void_p(coef.data_ptr()), None, C.c_void_p(gp or g.data_ptr()), C.byref(nnz), C.byref(objl))

    for fn in ("skml_glm_gradient_segmented_f64", "skml_glm_gradient_segmented_f32"):
        for kw in (dict(col_ptr=None), dict(batch=0), dict(gp=d.csc_val)):
            assert call(fn, **kw) == L.SKML_E_ARG and L.last_error(), f"{fn}, {kw}"
    torch.cuda.synchronize()
    assert bool((g == mark).all()) and bool((coef == mark).all()) and (nnz.value, objl.value) == (-7, -7.0)
    assert call("skml_glm_gradient_segmented_f64") == 0 and nnz.value > 0
