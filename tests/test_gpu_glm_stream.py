"""Stream ordering of the mini-batch gradient entries, in pattern A of tests/test_gpu_stream_order.py
(whose delay, fixtures and run_a this file uses): the context sits on a non-blocking stream, a
calibrated sleep is queued ahead of the copies that bring the fresh weight, labels and gradient in,
and clones of the outputs are queued behind the call.  Work that is not ordered after the stream
reads the stale inputs and is overwritten by the stale result; work that is not joined into the
stream is missed by the clones.  The reference is tests/glm_ref.py on the fresh data (the square
loss, whose every bit is pinned)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import glm_fixtures as FX
import glm_ref as R
from test_gpu_glm import _same
from test_gpu_stream_order import _drain, _ptr, run_a, sl  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_gradient(gpu, sl, dt):
    from sketchml_amd.data import DataSet
    data, dim = FX.lengths_data("mid")
    rows_n = len(data[3])
    ds = DataSet.fromCSR(*data, dim, device="cuda")
    d = ds.glm_data()
    npdt = np.float32 if dt == "f32" else np.float64
    w_fresh, w_stale = FX.weights(dim, npdt), FX.weights(dim, npdt, seed=77)
    y_fresh, y_stale = data[3], -3.0 * data[3]
    w, label = torch.from_numpy(w_stale.copy()).cuda(), ds.label
    label.copy_(torch.from_numpy(y_stale))
    r0, batch = 250, 120  # wraps
    pre, coef, loss = (torch.zeros(batch, dtype=torch.float64, device="cuda") for _ in range(3))
    grad = torch.zeros(dim, dtype=torch.float64, device="cuda")
    nnz, obj = C.c_int64(), C.c_double()
    fn = "skml_glm_gradient_f32" if dt == "f32" else "skml_glm_gradient_f64"

    def call(h):
        sl.c(fn, h, C.byref(d), r0, batch, R.L2_SQUARE, _ptr(w), _ptr(pre), _ptr(coef), _ptr(loss), _ptr(grad), C.byref(nnz),
             C.byref(obj))

    got = run_a(sl, [(w, torch.from_numpy(w_fresh).cuda()), (label, torch.from_numpy(y_fresh).cuda())], call,
                lambda: [pre, coef, loss, grad], scribble=[pre, coef, loss, grad], host_sync=True)
    rows, _ = R.window_rows(rows_n, r0, batch)
    r_pre, r_coef, r_loss = R.predict(data, w_fresh, rows, R.L2_SQUARE)
    g_ref = R.plus_by(data, dim, rows, r_coef)
    for a, b, what in zip(got, (r_pre, r_coef, r_loss, g_ref), ("pre", "coef", "loss", "grad_out")):
        _same(a.cpu().numpy(), b, what)
    # the two scalars come back through the synchronisation, so they are the fresh data's too
    assert nnz.value == R.count_nnz(g_ref)
    assert abs(obj.value - math.fsum(r_loss)) <= (batch - 1) * 2.0 ** -53 * math.fsum(np.abs(r_loss))


@pytest.mark.parametrize("form,dt", [("dense", "f64"), ("kv", "f32")])
def test_finish(gpu, sl, form, dt):
    n, dim = 40005, 40005 if form == "dense" else 90001
    rng = np.random.default_rng(8)
    npdt = np.float32 if dt == "f32" else np.float64
    v_fresh, v_stale = rng.standard_normal(n), 3.0 * rng.standard_normal(n) + 1.0
    w_fresh, w_stale = FX.weights(dim, npdt, seed=3) * 4096, FX.weights(dim, npdt, seed=4) * 4096
    k_fresh = np.sort(rng.choice(dim, n, replace=False)).astype(np.int32)
    k_stale = np.sort(rng.choice(dim, n, replace=False)).astype(np.int32)
    g, w, keys = torch.from_numpy(v_stale.copy()).cuda(), torch.from_numpy(w_stale.copy()).cuda(), torch.from_numpy(k_stale).cuda()
    g_src = torch.from_numpy(v_fresh).cuda()
    times, lam = 1.0 / 3.0, 0.0625

    def call(h):
        if form == "dense":
            sl.c("skml_glm_finish_dense_f64", h, _ptr(g), n, times, R.REG_L2, lam, _ptr(w), int(dt == "f32"))
        else:
            sl.c("skml_glm_finish_kv_f64", h, _ptr(keys), _ptr(g), n, dim, times, R.REG_L2, lam, _ptr(w), int(dt == "f32"))

    inputs = [(g, g_src), (w, torch.from_numpy(w_fresh).cuda())]
    if form == "kv":
        inputs.append((keys, torch.from_numpy(k_fresh).cuda()))
    # the entry works in place: the warm-up leaves a finished stale gradient, the fresh copy replaces it
    got = run_a(sl, inputs, call, lambda: [g])
    _same(got[0].cpu().numpy(), R.finish(k_fresh if form == "kv" else None, v_fresh, times, R.REG_L2, lam, w_fresh), form)
