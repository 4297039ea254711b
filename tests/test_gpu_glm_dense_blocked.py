"""The dense mini-batch gradient in the blocked summation order (skml_glm_gradient_dense_*blocked_*,
optim.batch_gradient(order="blocked")) over the four storages of x.  Shapes are placed around the plan's boundaries,
which are read from skml_debug_glm_dense_blocked_plan.  Narrow data sets are [:, :dim] views of NaN-filled buffers
(as tests/test_gpu_glm_dense_lowp.py builds them), so a pad element that reached a sum would show as NaN.

The exact test: x, w and labels are integers of magnitude <= 8, so every product and partial sum is an integer far
below 2^53 in any order (|g| <= 8 (8 * 8 * dim + 8) batch < 2^37 for the dim <= 4,112 and batch <= 513 used), and
every output equals the int64 numpy result bit for bit.  The rounded test: the reference is exact integer
arithmetic (every float is an integer times 2^-1100; Python ints through numpy object arrays), and the bounds are
those of any order of n fused or rounded terms, gamma_n = n u / (1 - n u), u = 2^-53."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import glm_ref as R
from sketchml_amd import _lib as L
from test_gpu_glm_dense import _loss, _same

pytestmark = pytest.mark.gpu
TYPES = {"f64": (None, 8), "f32": (torch.float32, 4), "bf16": (torch.bfloat16, 2), "f16": (torch.float16, 2)}
K = 1100  # every finite double is an integer times 2^-1074


def _ds(t, x, label):
    """x (rows x dim float64, exact in type t) as a DenseDataSet of storage t on the device; the pad is NaN."""
    from sketchml_amd.data import DenseDataSet
    dt, xb = TYPES[t]
    if dt is None:
        return DenseDataSet.fromArray(x, label, x.shape[1], device="cuda")
    buf = torch.full((x.shape[0], -(-x.shape[1] * xb // 16) * 16 // xb), float("nan"), dtype=dt, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x).to(dt).cuda()
    ds = DenseDataSet.fromArray(buf[:, :x.shape[1]], label, x.shape[1], device="cuda", xDtype=dt)
    assert ds.glm_data().x == buf.data_ptr() and ds.pitch == buf.shape[1]
    return ds


def _run(t, x, label, w, r0, batch, kind, order="blocked"):
    from sketchml_amd import optim
    out = optim.batch_gradient(torch.from_numpy(w).cuda(), _ds(t, x, label), r0, batch, _loss(kind), want_pre=True, order=order)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


def _exact_shapes(t):
    """(dim, batch) around every boundary of the plan: each L's edge, dim 1, odd and padded dims, long rows that end
    inside a group (a double x then starts its rows off 16 bytes: 8-byte loads) and long rows of whole groups (16-byte
    loads of x and w in every storage), each unsplit and split over waves, batch 1, RB - 1, RB, RB + 1, NB = 1, 2, 3, a
    batch that ends mid-unroll."""
    xb = TYPES[t][1]
    e, rb = 16 // xb, L.glm_dense_blocked_plan(xb, 1, 1)[3]
    dims = [1] + [e * lanes + d for lanes in (8, 16, 32, 64) for d in (-1, 0, 1)] + [e * 64 * 3 + 5, e * 195]
    batches = [1, rb - 1, rb, rb + 1, 2 * rb + 1, 37, 2]
    shapes = [(d, batches[i % len(batches)]) for i, d in enumerate(dims)] + [(3, b) for b in batches] + [(e * 512 + 3, 3), (e * 514, 3)]
    plans = [L.glm_dense_blocked_plan(xb, b, d) for d, b in shapes]
    assert {p[0] for p in plans} == {8, 16, 32, 64} and {p[4] for p in plans} == {1, 2, 3}
    for whole in (False, True):  # long rows, with and without a last partial group, unsplit and split
        assert {p[1] > 1 for (d, _), p in zip(shapes, plans) if d > 64 * e and (d % e == 0) == whole} == {False, True}
    return [(t, d, b) for d, b in shapes]


@pytest.mark.parametrize("t,dim,batch", [s for t in TYPES for s in _exact_shapes(t)])
def test_integer_data_equal_the_int64_result_bit_for_bit(gpu, t, dim, batch):
    rng, rows = np.random.default_rng(dim * 1000 + batch), batch + 2
    x, w = rng.integers(-8, 9, (rows, dim)), rng.integers(-8, 9, dim)
    win = np.r_[rows - 1, 0:batch - 1]  # from the last row on: the wrap falls inside the first block
    for kind, label in ((R.L2_HINGE, rng.choice([-1, 1], rows)), (R.L2_SQUARE, rng.integers(-8, 9, rows))):
        out = _run(t, x.astype(np.float64), label.astype(np.float64), w.astype(np.float64), rows - 1, batch, kind)
        pre = x[win] @ w
        loss = np.array([R.loss_of(kind, p, y) for p, y in zip(pre, label[win])])
        coef = np.array([-1.0 * R.grad_of(kind, p, y) for p, y in zip(pre, label[win])])
        g = x[win].T @ coef.astype(np.int64)
        for name, want in (("pre", pre), ("coef", coef), ("loss", loss), ("grad", g)):
            _same(out[name], want, name)
        assert out["nnz"] == np.count_nonzero(g) and out["objLoss"] == loss.sum()


def _ints(a):
    """a * 2^K as Python ints, exactly."""
    return np.array([n * ((1 << K) // d) for n, d in (float(v).as_integer_ratio() for v in np.ravel(a))], dtype=object).reshape(np.shape(a))


@functools.lru_cache(maxsize=None)
def _rounded(t, rows, dim):
    rng, e = np.random.default_rng(rows * 1000 + dim), 8 if t == "f16" else 12
    x = rng.standard_normal((rows, dim)) * np.exp2(rng.integers(-e, e + 1, (rows, dim)).astype(np.float64))
    if TYPES[t][0] is not None:
        x = torch.from_numpy(x).to(TYPES[t][0]).double().numpy()
    w = rng.standard_normal(dim) * np.exp2(rng.integers(-4, 5, dim).astype(np.float64))
    label = np.where(rng.random(rows) < 0.5, 1.0, -1.0)
    return x, label, w, _ints(x)


def _within(got, exact, mag, n, what):
    """|got - exact| <= gamma_n * mag, in exact arithmetic (exact and mag scaled by 2^2K)."""
    gamma = Fraction(n, 2 ** 53) / (1 - Fraction(n, 2 ** 53))
    err = [abs(Fraction(float(a)) * (1 << 2 * K) - b) for a, b in zip(got, exact)]
    print(f"{what}: the largest error is {max(float(e / (gamma * m)) for e, m in zip(err, mag) if m):.3g} of its bound")
    assert all(e <= gamma * m for e, m in zip(err, mag)), what


@pytest.mark.parametrize("t", list(TYPES))
@pytest.mark.parametrize("wdt,kind", [(np.float64, R.L2_LOG), (np.float32, R.L2_HINGE), (np.float64, R.L2_SQUARE)])
def test_rounded_data_within_the_bound_of_any_order(gpu, t, wdt, kind):
    e = 16 // TYPES[t][1]  # the second shape: long rows of whole groups (130 of them), some 25,000 elements in every storage
    assert L.glm_dense_blocked_plan(TYPES[t][1], 192 // e, e * 130)[:3] == (64, 1, 1)
    for rows, dim, batch in ((300, 70, 290), (192 // e, e * 130, 192 // e)):
        x, label, w, xi = _rounded(t, rows, dim)
        w = w.astype(wdt)
        out = _run(t, x, label, w, rows - 1, batch, kind)
        win = np.r_[rows - 1, 0:batch - 1]
        wi, ci = _ints(w.astype(np.float64)), _ints(out["coef"])
        _within(out["pre"], xi[win] @ wi, np.abs(xi[win]) @ np.abs(wi), dim, "pre")
        _within(out["grad"], xi[win].T @ ci, np.abs(xi[win]).T @ np.abs(ci), batch, "grad")  # given the device's own coef
        loss = np.array([R.loss_of(kind, p, y) for p, y in zip(out["pre"], label[win])])
        coef = np.array([-1.0 * R.grad_of(kind, p, y) for p, y in zip(out["pre"], label[win])])
        if kind == R.L2_LOG:
            assert np.all(np.abs(out["coef"] - coef) <= 2.0 ** -50 * np.abs(coef)) and np.all(np.abs(out["loss"] - loss) <= 2.0 ** -50 * (1.0 + np.abs(loss)))
        else:
            _same(out["coef"], coef, "coef")
            _same(out["loss"], loss, "loss")
        assert out["nnz"] == R.count_nnz(out["grad"])
        again = _run(t, x, label, w, rows - 1, batch, kind)  # determinism: the same call, the same bits
        assert all(np.array_equal(R.bits(out[k]), R.bits(again[k])) for k in ("pre", "coef", "loss", "grad")) and again["objLoss"] == out["objLoss"]


@pytest.mark.parametrize("t", list(TYPES))
def test_inf_row_and_the_smallest_call(gpu, t):
    x, label, w, _ = _rounded(t, 300, 70)
    x, w = x.copy(), w.copy()
    x[100, 9], w[9] = np.inf, 0.0
    with_row, without = _run(t, x, label, w, 50, 100, R.L2_SQUARE), _run(t, x, label, w, 101, 150, R.L2_SQUARE)
    assert np.isnan(with_row["pre"][50]) and np.isnan(with_row["pre"]).sum() == 1 and np.isnan(with_row["grad"]).all()  # Inf * 0
    assert all(np.isfinite(without[k]).all() for k in ("pre", "coef", "loss", "grad"))
    a, b = (_run(t, x[:3, :1], label[:3], w[:1], 2, 1, R.L2_SQUARE, order) for order in ("blocked", "sequential"))
    for k in ("pre", "coef", "loss", "grad"):
        _same(a[k], b[k], k)
    assert (a["nnz"], a["objLoss"]) == (b["nnz"], b["objLoss"])


def test_through_the_optimiser_and_the_model(gpu):
    import sketchml_amd as sk
    from sketchml_amd.optim import GradientDescent
    x, label, _, _ = _rounded("bf16", 300, 70)
    ds, w0, u = _ds("bf16", x, label), torch.zeros(70, dtype=torch.float64, device="cuda"), 2.0 ** -53
    grad, batch, obj, _ = GradientDescent(70, 0.1, 0.9, 0.9).miniBatchGradientDescent(w0, ds, _loss(R.L2_SQUARE), order="blocked")
    # w = 0: pre is +0.0 in any order and coef = -y exactly, so both sums lie within gamma_batch of the exact one
    want, mag = (x[:270].T @ -label[:270]) / 270, (np.abs(x[:270]).T @ np.abs(label[:270])) / 270
    # timesBy(1 / 270) rounds the factor and the product, numpy's division rounds once: 3 u more, 4 u allowed
    assert batch == 270 and np.isfinite(obj) and grad.values.numel() == 70
    assert np.all(np.abs(grad.values.cpu().numpy() - want) <= (2 * 270 * u / (1 - 270 * u) + 4 * u) * mag)
    conf = sk.MLConf(sk.LinearRegModel.name, "", "csv", 1, 70, epochNum=1, batchSpRatio=0.25, learnRate=0.1, l2Reg=0.0, compressor="None")
    mdl = sk.LinearRegModel(conf, _ds("bf16", x, label), _ds("bf16", x[:70], label[:70]), gradientOrder="blocked")
    tl, vl, _ = mdl.train()
    assert np.isfinite(tl + vl).all() and bool(torch.isfinite(mdl.weights).all()) and bool(mdl.weights.any())
    sparse = sk.DataSet.fromRows([(1.0, [0], [1.0])] * 3, 70, device="cuda")
    with pytest.raises(sk.SketchMLException, match="not built here"):
        GradientDescent(70, 0.1, 0.9, 0.9).miniBatchGradientDescent(w0, sparse, _loss(R.L2_SQUARE), order="blocked")
    with pytest.raises(sk.SketchMLException):
        GradientDescent(70, 0.1, 0.9, 0.9).miniBatchGradientDescent(w0, ds, _loss(R.L2_SQUARE), order="tree")


@pytest.mark.parametrize("t", ["f64", "bf16"])
def test_refusals_leave_the_outputs_untouched(gpu, t):
    from sketchml_amd.context import get_context
    x, label, w, _ = _rounded(t, 300, 70)
    ds, wd, mark = _ds(t, x, label), torch.from_numpy(w).cuda(), 123.456
    grad, coef = (torch.full((n,), mark, dtype=torch.float64, device="cuda") for n in (70, 300))
    nnz, obj, lowp = C.c_int64(-7), C.c_double(-7.0), t != "f64"
    d = ds.glm_data()

    def call(fn, row0=0, batch=10, g=None, **edit):
        data = type(d)(**{**{f: getattr(d, f) for f, _ in d._fields_}, **edit})
        return getattr(L.lib, fn)(get_context().handle, C.byref(data), row0, batch, R.L2_SQUARE, C.c_void_p(wd.data_ptr()), None,
                                  C.c_void_p(coef.data_ptr()), None, C.c_void_p(g or grad.data_ptr()), C.byref(nnz), C.byref(obj))

    bad = [dict(x=None), dict(batch=0), dict(g=ds.x.data_ptr())] + ([dict(x_kind=3), dict(pitch=64)] if lowp else [])
    for fn in ["skml_glm_gradient_dense_%sblocked_%s" % ("lowp_" if lowp else "", s) for s in ("f64", "f32")]:
        for kw in bad:
            assert call(fn, **kw) == L.SKML_E_ARG and L.last_error(), f"{fn}, {kw}"
    torch.cuda.synchronize()
    assert bool((grad == mark).all()) and bool((coef == mark).all()) and (nnz.value, obj.value) == (-7, -7.0)
    assert call("skml_glm_gradient_dense_%sblocked_f64" % ("lowp_" if lowp else "")) == 0 and nnz.value > 0
