"""The dense mini-batch gradient of K <= 16 models per pass on the fp64 matrix instruction
(skml_glm_gradient_dense_*multi_*, optim.batch_gradient_multi) over the four storages of x.  Shapes are placed around
the plan's boundaries, which are read from skml_debug_glm_dense_multi_plan.  Narrow data sets are [:, :dim] views of
NaN-filled buffers (tests/test_gpu_glm_dense_blocked.py's _ds), so a pad element that reached a sum would show as NaN.

The exact test: x, w and labels are integers of magnitude <= 8, so every product and partial sum is an integer far
below 2^53 in any order (|g| <= 8 (8 * 8 * dim + 8) batch < 2^41 for the dim <= 300 and batch <= 65,541 used), and
every output equals the int64 numpy result bit for bit; every model has its own w and labels, so a swapped model, row
or column index cannot cancel.  The rounded test: the reference is exact integer arithmetic and the bounds are those of
any order of n fused or rounded terms, gamma_n = n u / (1 - n u), u = 2^-53, as in the blocked order's test."""
import ctypes as C

import numpy as np
import pytest
import torch

import glm_ref as R
from sketchml_amd import _lib as L
from test_gpu_glm_dense import _loss, _same
from test_gpu_glm_dense_blocked import TYPES, _ds, _ints, _rounded, _within

pytestmark = pytest.mark.gpu
OUT = ("pre", "coef", "loss", "grad")


def _run(t, x, label, w, r0, batch, kind, labels=None):
    from sketchml_amd import optim
    lab = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float64)).cuda()
    out = optim.batch_gradient_multi(torch.from_numpy(w).cuda(), _ds(t, x, label), r0, batch, _loss(kind), labels=lab, want_pre=True)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


def _exact_shapes(t):
    """(K, dim, batch) around every boundary of the plan: dim 1, 3, 4, 5, one lane-step and one wave-step +- 1, one
    strip of the column sum +- 1 (odd dims for doubles, padded pitches for a narrow x); batch 1, 15, 16, 17, RB - 1, RB,
    RB + 1, NB = 1, 2, 3; a long row of few rows that is split over waves (S > 1), ending inside a lane-step and on a
    whole wave-step; enough tiles for R = 4, ending inside a tile; K = 1, 2, 15, 16."""
    xb = TYPES[t][1]
    ks = (1, 2, 15, 16)
    e, strip = L.glm_dense_multi_plan(xb, 1, 1, 1)[3:5]
    dims = [1, 3, 4, 5, e - 1, e + 1, 4 * e - 1, 4 * e, 4 * e + 1, strip - 1, strip + 1, 2 * strip + e + 1]
    shapes = [(ks[i % 4], d, (1, 15, 16, 17, 37)[i % 5]) for i, d in enumerate(dims)]
    for i, k in enumerate(ks):
        rb = L.glm_dense_multi_plan(xb, k, 1, 3)[5]
        shapes += [(k, 3, (rb - 1, rb, rb + 1, 2 * rb + 1)[(i + d) % 4]) for d in (0, 1)]
    shapes += [(16, 3, L.glm_dense_multi_plan(xb, 16, 1, 3)[5] + 1), (15, 4 * e * 9 + 3, 3), (2, 4 * e * 8, 18), (2, 5, 65536 + 5), (16, e + 1, 65536)]
    plans = [L.glm_dense_multi_plan(xb, k, b, d) for k, d, b in shapes]
    assert {p[1] for p in plans} == {1, 4} and {p[2] for p in plans} >= {1, 4} and {p[6] for p in plans} >= {1, 2, 3}
    return [(t, k, d, b) for k, d, b in shapes]


@pytest.mark.parametrize("t,models,dim,batch", [s for t in TYPES for s in _exact_shapes(t)])
def test_integer_data_equal_the_int64_result_bit_for_bit(gpu, t, models, dim, batch):
    rng, rows = np.random.default_rng(dim * 1000 + batch + models), batch + 2
    x, w = rng.integers(-8, 9, (rows, dim)), rng.integers(-8, 9, (models, dim))
    win = np.r_[rows - 1, 0:batch - 1]  # from the last row on: the wrap falls inside the first tile and the first block
    for kind, labels in ((R.L2_HINGE, rng.choice([-1, 1], (models, rows))), (R.L2_SQUARE, rng.integers(-8, 9, (models, rows)))):
        out = _run(t, x.astype(np.float64), labels[0].astype(np.float64), w.astype(np.float64), rows - 1, batch, kind, labels)
        pre, y = (w @ x[win].T).astype(np.float64), labels[:, win].astype(np.float64)
        if kind == R.L2_HINGE:  # Loss.scala's branches; -1.0 * 0.0 is -0.0 on the device too
            loss, coef = np.where(pre * y < 1, 1 - pre * y, 0.0), -1.0 * np.where(pre * y <= 1, y, 0.0)
        else:
            loss, coef = (0.5 * (pre - y)) * (pre - y), -1.0 * (y - pre)
        g = coef.astype(np.int64) @ x[win]
        for name, want in (("pre", pre), ("coef", coef), ("loss", loss), ("grad", g)):
            _same(out[name], np.asarray(want, dtype=np.float64), name)
        assert out["nnz"] == [int(np.count_nonzero(r)) for r in g] and out["objLoss"] == [float(r.sum()) for r in loss]


def test_labels_none_is_the_data_sets_label_for_every_model(gpu):
    x, label, w, _ = _rounded("f32", 300, 70)
    ws = np.stack([w, -w, 0.5 * w])
    a, b = _run("f32", x, label, ws, 290, 40, R.L2_LOG), _run("f32", x, label, ws, 290, 40, R.L2_LOG, np.stack([label] * 3))
    assert all(np.array_equal(R.bits(a[k]), R.bits(b[k])) for k in OUT) and (a["nnz"], a["objLoss"]) == (b["nnz"], b["objLoss"])


@pytest.mark.parametrize("t", list(TYPES))
@pytest.mark.parametrize("wdt,kind", [(np.float64, R.L2_LOG), (np.float32, R.L1_LOG), (np.float32, R.L2_HINGE), (np.float64, R.L2_SQUARE)])
def test_rounded_data_within_the_bound_of_any_order(gpu, t, wdt, kind):
    e = 16 // TYPES[t][1]  # the shapes of the blocked order's test: several tiles and two blocks at K = 3; long rows at K = 16
    for models, (rows, dim, batch) in ((3, (300, 70, 290)), (16, (192 // e, e * 130, 192 // e))):
        x, label, w, xi = _rounded(t, rows, dim)
        rng = np.random.default_rng(models)
        ws = (w[None, :] * rng.standard_normal((models, dim))).astype(wdt)
        labels = np.where(rng.random((models, rows)) < 0.5, 1.0, -1.0)
        out = _run(t, x, label, ws, rows - 1, batch, kind, labels)
        win = np.r_[rows - 1, 0:batch - 1]
        for m in range(models):
            wi, ci = _ints(ws[m].astype(np.float64)), _ints(out["coef"][m])
            _within(out["pre"][m], xi[win] @ wi, np.abs(xi[win]) @ np.abs(wi), dim, f"pre[{m}]")
            _within(out["grad"][m], xi[win].T @ ci, np.abs(xi[win]).T @ np.abs(ci), batch, f"grad[{m}]")  # given the device's own coef
            loss = np.array([R.loss_of(kind, p, y) for p, y in zip(out["pre"][m], labels[m, win])])
            coef = np.array([-1.0 * R.grad_of(kind, p, y) for p, y in zip(out["pre"][m], labels[m, win])])
            if kind in (R.L1_LOG, R.L2_LOG):
                assert np.all(np.abs(out["coef"][m] - coef) <= 2.0 ** -50 * np.abs(coef))
                assert np.all(np.abs(out["loss"][m] - loss) <= 2.0 ** -50 * (1.0 + np.abs(loss)))
            else:
                _same(out["coef"][m], coef, "coef")
                _same(out["loss"][m], loss, "loss")
            assert out["nnz"][m] == R.count_nnz(out["grad"][m])
        again = _run(t, x, label, ws, rows - 1, batch, kind, labels)  # determinism: the same call, the same bits
        assert all(np.array_equal(R.bits(out[k]), R.bits(again[k])) for k in OUT) and again["objLoss"] == out["objLoss"]


@pytest.mark.parametrize("t", list(TYPES))
def test_inf_row_reaches_its_pre_and_its_windows_grad_only(gpu, t):
    x, label, w, _ = _rounded(t, 300, 70)
    x, ws = x.copy(), np.stack([w, 2 * w, -w])
    x[100, 9], ws[:, 9] = np.inf, 0.0
    with_row, without = _run(t, x, label, ws, 50, 100, R.L2_SQUARE), _run(t, x, label, ws, 101, 150, R.L2_SQUARE)
    assert np.isnan(with_row["pre"][:, 50]).all() and np.isnan(with_row["pre"]).sum() == 3 and np.isnan(with_row["grad"]).all()  # Inf * 0
    assert all(np.isfinite(without[k]).all() for k in OUT)


@pytest.mark.parametrize("t", ["f64", "bf16"])
def test_outputs_end_at_k_and_batch_and_refusals_leave_them_untouched(gpu, t):
    from sketchml_amd.context import get_context
    x, label, w, _ = _rounded(t, 300, 70)
    models, batch, mark = 3, 37, 123.456
    ds, wd = _ds(t, x, label), torch.from_numpy(np.stack([w] * 17)).cuda()
    grad = torch.full((17 * 70 + 8,), mark, dtype=torch.float64, device="cuda")
    pre, coef, loss = (torch.full((17 * batch + 8,), mark, dtype=torch.float64, device="cuda") for _ in range(3))
    nnz, obj, lowp = (C.c_int64 * 17)(*[-7] * 17), (C.c_double * 17)(*[-7.0] * 17), t != "f64"
    d = ds.glm_data()

    def call(fn, row0=0, batch=batch, models=models, g=None, **edit):
        data = type(d)(**{**{f: getattr(d, f) for f, _ in d._fields_}, **edit})
        return getattr(L.lib, fn)(get_context().handle, C.byref(data), row0, batch, R.L2_SQUARE, models, C.c_void_p(wd.data_ptr()), None,
                                  C.c_void_p(pre.data_ptr()), C.c_void_p(coef.data_ptr()), C.c_void_p(loss.data_ptr()),
                                  C.c_void_p(g or grad.data_ptr()), nnz, obj)

    bad = [dict(models=0), dict(models=17), dict(g=ds.x.data_ptr()), dict(g=coef.data_ptr() + 8 * batch), dict(x=None), dict(batch=0),
           dict(batch=301), dict(row0=300)] + ([dict(x_kind=3), dict(pitch=64)] if lowp else [])
    names = ["skml_glm_gradient_dense_%smulti_%s" % ("lowp_" if lowp else "", s) for s in ("f64", "f32")]
    for fn in names:
        for kw in bad:
            assert call(fn, **kw) == L.SKML_E_ARG and L.last_error(), f"{fn}, {kw}"
    torch.cuda.synchronize()
    assert all(bool((a == mark).all()) for a in (grad, pre, coef, loss)) and list(nnz) == [-7] * 17 and list(obj) == [-7.0] * 17
    assert call(names[0]) == 0  # models past K and rows past batch: the bytes behind the outputs keep the canary
    for a, n in ((grad, models * 70), (pre, models * batch), (coef, models * batch), (loss, models * batch)):
        assert bool((a[:n] != mark).all()) and bool((a[n:] == mark).all())
    assert all(v >= 0 for v in nnz[:models]) and list(nnz[models:]) == [-7] * 14 and list(obj[models:]) == [-7.0] * 14


def test_through_the_interface(gpu):
    import sketchml_amd as sk
    from sketchml_amd import optim
    from sketchml_amd.data import one_vs_rest_labels
    from sketchml_amd.gradient import DenseDoubleGradient
    x, label, w, _ = _rounded("bf16", 300, 70)
    ds, rng = _ds("bf16", x, label), np.random.default_rng(5)
    ws = torch.from_numpy(w[None, :] * rng.standard_normal((20, 70))).cuda()
    y = one_vs_rest_labels(rng.integers(0, 20, 300), list(range(20)), "cuda")
    assert one_vs_rest_labels([2, 0, 2], [0, 2], "cuda").tolist() == [[-1.0, 1.0, -1.0], [1.0, -1.0, 1.0]]
    loss = _loss(R.L2_LOG)
    whole = optim.batch_gradient_multi(ws, ds, 280, 50, loss, labels=y, want_pre=True)  # K = 20: groups of 16 and 4
    parts = [optim.batch_gradient_multi(ws[a:b], ds, 280, 50, loss, labels=y[a:b].contiguous(), want_pre=True) for a, b in ((0, 16), (16, 20))]
    for k in OUT:
        assert whole[k].shape[0] == 20 and torch.equal(whole[k].view(torch.int64), torch.cat([p[k] for p in parts]).view(torch.int64))
    assert whole["nnz"] == parts[0]["nnz"] + parts[1]["nnz"] and whole["objLoss"] == parts[0]["objLoss"] + parts[1]["objLoss"]

    gd, index = optim.GradientDescent(70, 0.1, 0.9, 0.5), ds.readIndex
    res = gd.miniBatchGradientDescentMulti(ws[:3], ds, loss, labels=y[:3].contiguous())
    assert ds.readIndex == (index + 150) % 300 and gd.batch == 1 and len(res) == 3
    raw = optim.batch_gradient_multi(ws[:3], ds, index, 150, loss, labels=y[:3].contiguous())
    for m, (grad, size, obj, reg) in enumerate(res):
        want = DenseDoubleGradient(70, raw["grad"][m].clone())
        optim.finish_gradient(want, 1.0 / 150, loss, ws[m])
        assert size == 150 and obj == raw["objLoss"][m] and reg == float(loss.getReg(ws[m]))
        assert torch.equal(grad.values.view(torch.int64), want.values.view(torch.int64))
    sparse = sk.DataSet.fromRows([(1.0, [0], [1.0])] * 3, 70, device="cuda")
    for f in (lambda: optim.batch_gradient_multi(ws, sparse, 0, 1, loss), lambda: gd.miniBatchGradientDescentMulti(ws, sparse, loss)):
        with pytest.raises(sk.SketchMLException, match="not built here"):
            f()
